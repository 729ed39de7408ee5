"""Input feed rate: the serial host generator (input_reader.batches + .to(dev)) against the asynchronous pipeline
(mtl_ssl_amd.input_pipeline), on synthetic VOC- or COCO-like JPEG records written with the converters' own writer
(create_mscoco_tf_record.example_from_image: boxes, windows, closeness, 2x64x64 edge masks).

    python tools/input_feed_rate.py --config configs/frcnn_resnet101_coco_mtl.config --kind coco --out profiles/x.json

Reports, in one JSON document:
  host      the machine's per-core speed (one resize_bilinear_legacy 375x500 -> 600x800 and a fixed numpy loop), PIL's
            JPEG decode time on the records' photo-like images, the tf.Example parse time with and without edge masks;
  feed      images/s of each feed alone (device synchronised at the end) and the async pipeline's per-stage times
            (parse / decode in the workers, staging in the consumer, H2D copy / prepare kernel on the device);
  train     ms/step of the configuration fed from records by each feed, and on synthetic device batches of the same
            shape in the same process. The training records are all landscape (one resized shape, the synthetic one).
With --augment, the feed and train sections also report the feeds with AUGMENT (normalize to [0, 1], flip,
random_distort_color, random_pixel_value_scale, random_black_patches, normalize back) as host_augment /
async_augment, beside the flip-only ones from the same run (the augmented host generator is timed on fewer
batches, and in the feed section only).
Not part of bench.py."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"voc": [(375, 500), (500, 375), (333, 500)], "coco": [(480, 640), (640, 427)]}   # (H, W)


def photo(rng, H, W):
    """A photo-like image: smooth colour fields, a few edges and mild sensor noise (JPEG sizes like natural photos'
    tens of KB, unlike white noise)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.zeros((H, W, 3), np.float32)
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = rng.uniform(0.002, 0.02, 2).tolist() + [rng.uniform(0, 6.3)]
            img[..., c] += rng.uniform(20, 60) * np.sin(fy * y * 6.3 + fx * x * 6.3 + ph)
    for _ in range(6):
        y0, x0 = rng.randint(0, H), rng.randint(0, W)
        img[y0:y0 + rng.randint(20, H // 2), x0:x0 + rng.randint(20, W // 2)] += rng.uniform(-60, 60, 3)
    img += 128 + rng.normal(0, 4, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def write_records(path, n, shapes, K, seed):
    from PIL import Image
    from mtl_ssl_amd import create_mscoco_tf_record as C
    from mtl_ssl_amd import input_reader as R
    rng = np.random.RandomState(seed)
    recs, jpegs = [], []
    for i in range(n):
        H, W = shapes[i % len(shapes)]
        buf = io.BytesIO()
        Image.fromarray(photo(rng, H, W)).save(buf, format="JPEG", quality=90)
        G = int(rng.randint(1, 6))
        anns = [{"bbox": [float(rng.uniform(0, W * 0.6)), float(rng.uniform(0, H * 0.6)), float(rng.uniform(20, W * 0.4)),
                          float(rng.uniform(20, H * 0.4))], "category_id": int(rng.randint(1, K + 1))} for _ in range(G)]
        recs.append(C.example_from_image({"file_name": "im%05d.jpg" % i, "id": i}, anns, {}, buf.getvalue(), K, rng))
        jpegs.append(buf.getvalue())
    R.write_tfrecord(path, recs)
    return recs, jpegs


def host_speed(recs, jpegs):
    from PIL import Image
    from mtl_ssl_amd import input_reader as R
    from mtl_ssl_amd import preprocessor
    img = np.random.RandomState(0).uniform(0, 255, (375, 500, 3)).astype(np.float32)
    t = time.perf_counter()
    preprocessor.resize_bilinear_legacy(img, 600, 800)
    resize_ms = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    acc = 0
    for i in range(2_000_000):
        acc += i & 7
    py_ms = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    for j in jpegs:
        np.asarray(Image.open(io.BytesIO(j)).convert("RGB"))
    dec_ms = 1e3 * (time.perf_counter() - t) / len(jpegs)
    t = time.perf_counter()
    for r in recs:
        R.parse_example(r)
    parse_ms = 1e3 * (time.perf_counter() - t) / len(recs)
    stripped = []
    for r in recs:
        f = R.parse_example(r)
        for k in [k for k in f if k.startswith("image/edgemask/")]:
            del f[k]
        stripped.append(R.serialize_example(f))
    t = time.perf_counter()
    for r in stripped:
        R.parse_example(r)
    parse_plain_ms = 1e3 * (time.perf_counter() - t) / len(recs)
    return {"cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
            "resize_bilinear_legacy_375x500_to_600x800_ms": resize_ms, "python_loop_2M_ms": py_ms,
            "pil_jpeg_decode_ms_per_image": dec_ms, "mean_jpeg_kb": sum(map(len, jpegs)) / len(jpegs) / 1024,
            "tf_example_parse_ms": parse_ms, "tf_example_parse_without_edgemask_ms": parse_plain_ms,
            "edgemask_parse_ms": parse_ms - parse_plain_ms}


FLIP_ONLY = "train_config { data_augmentation_options { random_horizontal_flip { } } }"
AUGMENT = """train_config {
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 255 target_minval: 0 target_maxval: 1 } }
  data_augmentation_options { random_horizontal_flip { } }
  data_augmentation_options { random_distort_color { } }
  data_augmentation_options { random_pixel_value_scale { } }
  data_augmentation_options { random_black_patches { } }
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 1 target_minval: 0 target_maxval: 255 } }
}"""


def feed_kwargs(model_config, K, B, options=FLIP_ONLY):
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
    rz = model_config.faster_rcnn.image_resizer
    from mtl_ssl_amd import config
    opts = config.parse_pipeline_config(options).train_config.data_augmentation_options
    return dict(num_classes=K, batch_size=B, augmentation_options=opts, loop=True, shuffle_buffer=16,
                resized_shape=lambda h, w: M.resized_shape(h, w, rz))


def make_feed(kind, path, dev, kw, seed, workers=None, profile=False):
    from mtl_ssl_amd import input_pipeline
    from mtl_ssl_amd.train import record_batches
    k = dict(kw)
    K, B, opts = k.pop("num_classes"), k.pop("batch_size"), k.pop("augmentation_options")
    rng = np.random.RandomState(seed)
    if kind == "host":
        return record_batches("host", [path], K, B, opts, rng, dev, {}, **k)
    return input_pipeline.InputPipeline([path], K, B, opts, rng, device=dev, num_workers=workers, profile=profile, **k)


def feed_only(path, dev, feeds, batches, workers):
    """feeds: {name: (host | async, feed kwargs, batches to time or None for `batches`)}."""
    import torch
    out = {}
    for name, (kind, kw, nb) in feeds.items():
        feed = make_feed(kind, path, dev, kw, 1, workers, profile=True)
        next(feed)                                 # worker start-up / first decode outside the timed region
        torch.cuda.synchronize()
        n, t = 0, time.perf_counter()
        for _ in range(nb or batches):
            n += next(feed)["images"].shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        row = {"images_per_s": n / dt, "images": n, "seconds": dt}
        if kind == "async":
            tm = feed.timings
            got = n + kw["batch_size"]
            c, p, nbytes, pix = feed.device_times()
            row.update(workers=feed.num_workers, worker_parse_ms_per_image=1e3 * tm["parse"] / got,
                       worker_decode_ms_per_image=1e3 * tm["decode"] / got,
                       consumer_stage_ms_per_batch=1e3 * tm["stage"] / max(1, feed._preparer.k),
                       h2d_copy_us_per_batch=1e6 * c / max(1, len(feed._preparer.timed)),
                       h2d_gb_per_s=nbytes / max(c, 1e-9) / 1e9,
                       prepare_kernel_us_per_batch=1e6 * p / max(1, len(feed._preparer.timed)),
                       prepare_kernel_out_gb_per_s=12 * pix / max(p, 1e-9) / 1e9)
            feed.close()
        out[name] = row
    return out


def train_rates(cfg_path, path, dev, feeds, steps, warmup, workers, HW):
    import torch
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(cfg_path).read())
    B, K = feeds["async"][1]["batch_size"], feeds["async"][1]["num_classes"]
    model = model_builder.build(cfg.model, True, dev, seed=0)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    out = {}

    def timed(next_batch):
        for _ in range(warmup):
            tr.step(next_batch())
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            tr.step(next_batch())
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t) / steps

    ring = [synthetic.make_batch(B, HW[0], HW[1], K, seed=1234 + 1000 * i, device=dev, max_gt=5, num_windows=64)
            for i in range(4)]
    it = iter(range(10 ** 9))
    out["synthetic_ms_per_step"] = timed(lambda: dict(ring[next(it) % 4]))
    for name, (kind, kw, _) in feeds.items():
        feed = make_feed(kind, path, dev, kw, 2, workers)
        out[name + "_ms_per_step"] = timed(lambda: next(feed))
        if hasattr(feed, "close"):
            feed.close()
    out["synthetic_ms_per_step_again"] = timed(lambda: dict(ring[next(it) % 4]))
    out["async_over_synthetic"] = out["async_ms_per_step"] / min(out["synthetic_ms_per_step"],
                                                               out["synthetic_ms_per_step_again"])
    if "async_augment" in feeds:
        out["async_augment_over_async"] = out["async_augment_ms_per_step"] / out["async_ms_per_step"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config"))
    ap.add_argument("--kind", choices=sorted(SHAPES), default="coco")
    ap.add_argument("--records", type=int, default=48)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--feed-batches", type=int, default=60)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--workers", type=int, default=None, help="decode workers (default: default_num_workers(8))")
    ap.add_argument("--skip", choices=("none", "feed", "train"), default="none")
    ap.add_argument("--workdir", default="/tmp/input_feed_rate")
    ap.add_argument("--out", default="")
    ap.add_argument("--augment", action="store_true", help="also time the feeds with the AUGMENT options")
    a = ap.parse_args(argv)
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mtl_ssl_amd import config, input_pipeline
    os.makedirs(a.workdir, exist_ok=True)
    cfg = config.parse_pipeline_config(open(a.config).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    dev = torch.device("cuda", 0)
    kw = feed_kwargs(cfg.model, K, a.batch)
    feeds = {"host": ("host", kw, None), "async": ("async", kw, None)}
    if a.augment:
        akw = feed_kwargs(cfg.model, K, a.batch, AUGMENT)
        feeds.update(host_augment=("host", akw, max(1, a.feed_batches // 6)), async_augment=("async", akw, None))
    mixed = os.path.join(a.workdir, "mixed.record")
    recs, jpegs = write_records(mixed, a.records, SHAPES[a.kind], K, 0)
    res = {"config": os.path.relpath(a.config, ROOT), "kind": a.kind, "shapes_hw": SHAPES[a.kind], "augment": a.augment,
           "records": a.records, "per_gpu_batch": a.batch,
           "default_workers": input_pipeline.default_num_workers(8, 1), "host": host_speed(recs, jpegs)}
    print(json.dumps(res["host"]), flush=True)
    if a.skip != "feed":
        res["feed"] = feed_only(mixed, dev, feeds, a.feed_batches, a.workers)
        print(json.dumps(res["feed"]), flush=True)
    if a.skip != "train":
        land = os.path.join(a.workdir, "landscape.record")
        write_records(land, a.records, SHAPES[a.kind][:1], K, 1)
        from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
        HW = M.resized_shape(*SHAPES[a.kind][0], cfg.model.faster_rcnn.image_resizer)
        train_feeds = {k: v for k, v in feeds.items() if k != "host_augment"}      # its feed rate says enough
        res["train"] = dict(train_rates(a.config, land, dev, train_feeds, a.steps, a.warmup, a.workers, HW), image_hw=HW,
                            steps=a.steps, warmup=a.warmup)
        print(json.dumps(res["train"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
