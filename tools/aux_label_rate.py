"""What generating the auxiliary labels on the device costs (Trainer(aux_labels="generate")).

    python tools/aux_label_rate.py --out profiles/aux_label_rate_configs1.json

Reports, in one JSON document:
  kernels   per-launch time (HIP events around a run of back-to-back launches) of the window draw and the three label
            kernels at the configuration's shapes (B images, 64 windows, K classes) for 8 and for 100 boxes per image;
  host      the host generator's time for the same batch (labels.random_windows + closeness_labels + edgemask, one
            process): what a user pays per step for fresh labels without the kernels;
  train     ms/step of the configuration fed from records (asynchronous pipeline) with aux_labels="record" and with
            "generate", in the same process, interleaved, several repeats with their spread.
Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make_gt(rng, B, G, K, dev):
    import torch
    cyx, hw = rng.uniform(0.1, 0.9, (B, G, 2)), rng.uniform(0.05, 0.5, (B, G, 2))
    boxes = np.concatenate([cyx - hw / 2, cyx + hw / 2], 2).clip(0, 1).astype(np.float32)
    ids = rng.randint(1, K + 1, (B, G))
    cls = np.zeros((B, G, K + 1), np.float32)
    for b in range(B):
        cls[b, np.arange(G), ids[b]] = 1
    return (boxes, ids, torch.from_numpy(boxes).to(dev), torch.from_numpy(cls).to(dev),
            torch.full((B,), G, dtype=torch.int32, device=dev))


def event_us(fn, launches, warmup=20):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def kernel_times(ops, dev, B, Wn, K, HW, launches):
    from mtl_ssl_amd import labels
    out = {}
    for G in (8, 100):
        rng = np.random.RandomState(G)
        boxes, ids, b, cl, num = make_gt(rng, B, G, K, dev)
        wb = ops.aux_draw_windows(b, num, Wn, HW, 1, 0, 0)
        row = {"draw_windows_us": event_us(lambda: ops.aux_draw_windows(b, num, Wn, HW, 1, 0, 0), launches),
               "window_labels_us": event_us(lambda: ops.aux_window_labels(b, cl, num, wb, HW), launches),
               "closeness_us": event_us(lambda: ops.aux_closeness(b, cl, num, HW), launches),
               "edgemask_us": event_us(lambda: ops.aux_edgemask(b, num, HW), launches)}
        row["sum_us"] = sum(row.values())
        # the host generator for the same batch (absolute boxes, the records' three-decimal labels)
        t = time.perf_counter()
        for i in range(B):
            ab = boxes[i].astype(np.float64) * [HW[0], HW[1], HW[0], HW[1]]
            labels.random_windows(ab, ids[i], HW[1], HW[0], K, np.random.RandomState(i), Wn)
            labels.closeness_labels(ab, ids[i], HW[1], HW[0], K)
            labels.edgemask(ab, HW[1], HW[0])
        row["host_generator_ms"] = 1e3 * (time.perf_counter() - t)
        out["boxes_%d" % G] = row
    return out


def train_times(cfg_path, workdir, dev, B, K, HW, steps, warmup, repeats, records):
    import torch
    import input_feed_rate as F
    from mtl_ssl_amd import config, model_builder, trainer
    cfg = config.parse_pipeline_config(open(cfg_path).read())
    land = os.path.join(workdir, "landscape.record")
    F.write_records(land, records, F.SHAPES["coco"][:1], K, 1)
    model = model_builder.build(cfg.model, True, dev, seed=0)
    trainers = {"record": trainer.Trainer(model, cfg.train_config, 1),
                "generate": trainer.Trainer(model, cfg.train_config, 1, aux_labels="generate")}
    feed = F.make_feed("async", land, dev, F.feed_kwargs(cfg.model, K, B), 2)
    times = {k: [] for k in trainers}
    try:
        for tr in trainers.values():
            for _ in range(warmup):
                tr.step(next(feed))
        for _ in range(repeats):
            for name, tr in trainers.items():
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(steps):
                    tr.step(next(feed))
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t) / steps)
    finally:
        feed.close()
    out = {"steps": steps, "warmup": warmup, "repeats": repeats, "image_hw": list(HW)}
    for name, v in times.items():
        out[name + "_ms_per_step"] = v
        out[name + "_mean_ms"] = float(np.mean(v))
        out[name + "_spread_ms"] = float(max(v) - min(v))
    out["generate_minus_record_ms"] = out["generate_mean_ms"] - out["record_mean_ms"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config"))
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--records", type=int, default=48)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--workdir", default="/tmp/aux_label_rate")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mtl_ssl_amd import config, ops
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
    if not torch.cuda.is_available():
        raise SystemExit("aux_label_rate needs a GPU: a CPU run says nothing about these times")
    os.makedirs(a.workdir, exist_ok=True)
    cfg = config.parse_pipeline_config(open(a.config).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    HW = M.resized_shape(480, 640, cfg.model.faster_rcnn.image_resizer)
    dev = torch.device("cuda", 0)
    res = {"config": os.path.relpath(a.config, ROOT), "per_gpu_batch": a.batch, "windows": a.windows, "classes": K,
           "image_hw": list(HW), "launches_per_timing": a.launches,
           "kernels": kernel_times(ops, dev, a.batch, a.windows, K, HW, a.launches)}
    print(json.dumps(res["kernels"]), flush=True)
    if not a.skip_train:
        res["train"] = train_times(a.config, a.workdir, dev, a.batch, K, HW, a.steps, a.warmup, a.repeats, a.records)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
