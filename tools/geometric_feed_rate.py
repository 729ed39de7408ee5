"""What random crop / pad augmentation costs in the input feed: the asynchronous pipeline with flip-only,
photometric-only and random_crop_pad_image + flip options on tools/input_feed_rate.py's COCO-like JPEG records, taken
interleaved in one process (run r times every configuration in turn; the median of the runs is reported beside them).

    python tools/geometric_feed_rate.py --out profiles/geometric_feed_rate.json

Reports the feed-alone images/s, the prepare-kernel time per batch (InputPipeline.device_times()), and the record-fed
ms/step of the configuration with aux_labels="generate" for flip-only against the geometric options, and says whether
the geometric feed still outruns the step. Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TO_UNIT = "normalize_image { original_minval: 0 original_maxval: 255 target_minval: 0 target_maxval: 1 }"
TO_255 = "normalize_image { original_minval: 0 original_maxval: 1 target_minval: 0 target_maxval: 255 }"
OPTIONS = {
    "flip": ["random_horizontal_flip { }"],
    "photometric": [TO_UNIT, "random_distort_color { }", "random_pixel_value_scale { }", TO_255],
    "geometric": ["random_crop_pad_image { }", "random_horizontal_flip { }"],
}


def _config_text(options):
    return "train_config { %s }" % " ".join("data_augmentation_options { %s }" % o for o in options)


def _feed(path, dev, kw, seed, workers, profile=False):
    from mtl_ssl_amd import input_pipeline
    k = dict(kw)
    K, B, opts = k.pop("num_classes"), k.pop("batch_size"), k.pop("augmentation_options")
    return input_pipeline.InputPipeline([path], K, B, opts, np.random.RandomState(seed), device=dev, num_workers=workers,
                                        profile=profile, geometric=True, **k)


def feed_run(path, dev, kw, batches, workers, seed):
    import torch
    with _feed(path, dev, kw, seed, workers, profile=True) as feed:
        next(feed)                                 # worker start-up / first decode outside the timed region
        torch.cuda.synchronize()
        n, t = 0, time.perf_counter()
        for _ in range(batches):
            n += next(feed)["images"].shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        _, p, _, _ = feed.device_times()
        return n / dt, 1e6 * p / max(1, len(feed._preparer.timed))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config"))
    ap.add_argument("--records", type=int, default=48)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--feed-batches", type=int, default=40)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--workdir", default="/tmp/geometric_feed_rate")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch
    import __graft_entry__ as ge
    ge.build()
    import input_feed_rate as F
    from mtl_ssl_amd import config, input_pipeline, model_builder, trainer
    os.makedirs(a.workdir, exist_ok=True)
    cfg = config.parse_pipeline_config(open(a.config).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    dev = torch.device("cuda", 0)
    kws = {name: F.feed_kwargs(cfg.model, K, a.batch, _config_text(o)) for name, o in OPTIONS.items()}
    mixed = os.path.join(a.workdir, "mixed.record")
    F.write_records(mixed, a.records, F.SHAPES["coco"], K, 0)
    res = {"config": os.path.relpath(a.config, ROOT), "shapes_hw": F.SHAPES["coco"], "records": a.records,
           "per_gpu_batch": a.batch, "runs": a.runs, "options": OPTIONS,
           "workers": a.workers or input_pipeline.default_num_workers(8, 1), "feed": {}, "train": {}}
    runs = {name: [] for name in OPTIONS}
    for r in range(a.runs):                                  # interleaved: every configuration in every round
        for name in OPTIONS:
            runs[name].append(feed_run(mixed, dev, kws[name], a.feed_batches, a.workers, 1 + r))
    for name, rows in runs.items():
        res["feed"][name] = {"images_per_s": statistics.median(x for x, _ in rows),
                             "prepare_kernel_us_per_batch": statistics.median(x for _, x in rows),
                             "images_per_s_runs": [x for x, _ in rows], "prepare_kernel_us_per_batch_runs": [x for _, x in rows]}
    print(json.dumps(res["feed"]), flush=True)

    model = model_builder.build(cfg.model, True, dev, seed=0)
    tr = trainer.Trainer(model, cfg.train_config, 1, aux_labels="generate")
    feeds = {name: _feed(mixed, dev, kws[name], 2, a.workers) for name in ("flip", "geometric")}
    steps = {name: [] for name in feeds}
    try:
        for r in range(a.runs):
            for name, feed in feeds.items():
                for _ in range(a.warmup):
                    tr.step(next(feed))
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.steps):
                    tr.step(next(feed))
                torch.cuda.synchronize()
                steps[name].append(1e3 * (time.perf_counter() - t) / a.steps)
    finally:
        for feed in feeds.values():
            feed.close()
    for name, rows in steps.items():
        res["train"][name] = {"ms_per_step": statistics.median(rows), "ms_per_step_runs": rows,
                              "images_per_s": 1e3 * a.batch / statistics.median(rows)}
    res["train"].update(aux_labels="generate", steps=a.steps, warmup=a.warmup,
                        note="mixed portrait / landscape records; the geometric batches have many resized shapes")
    ahead = res["feed"]["geometric"]["images_per_s"] / res["train"]["geometric"]["images_per_s"]
    res["geometric_feed_over_step_images_per_s"] = ahead
    res["geometric_feed_outruns_the_step"] = ahead > 1.0
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
