"""Inference rate of mtl_ssl_amd.inference.Detector on one GPU, for one configuration with its initial weights, written
to a state file like a trained checkpoint's (the convolutions do not depend on the values; the NMS work may).

    python tools/inference_rate.py --config configs/frcnn_resnet101_coco_mtl.config --out profiles/x.json

Reports, in one JSON document:
  latency_b1        ms per image of detect_images([one image]) at the source size --hw (600x1024 by default: the
                    keep-aspect resizer's output, so the prepare kernel resizes 1:1), HIP events around a synchronised
                    window of --iters calls after --warmup calls, plus the host's wall clock over the same window;
  group             images/s of detect_images on a same-size list of --group images (one group, one launch chain);
  encoded           images/s of detect_encoded on the same pictures as JPEG (host decode + the device path);
  host_decode       PIL's JPEG decode rate on those JPEGs (decode_image, one core), and their mean size.
Every detect_* call ends in a device-to-host copy of its detections, so each call is synchronised. Not part of
bench.py."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _timed(torch, fn, warmup, iters):
    """(device ms per call by HIP events, host ms per call) over a window opened and closed synchronised."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    return a.elapsed_time(b) / iters, wall


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config"))
    ap.add_argument("--hw", default="600x1024")
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    f = ap.parse_args(argv)
    import torch
    from PIL import Image
    from input_feed_rate import photo
    from mtl_ssl_amd import config, inference, model_builder, params
    H, W = (int(v) for v in f.hw.split("x"))
    cfg = config.parse_pipeline_config(open(f.config).read())
    rng = np.random.RandomState(0)
    pictures = [photo(rng, H, W) for _ in range(f.group)]
    jpegs = []
    for p in pictures:
        buf = io.BytesIO()
        Image.fromarray(p).save(buf, format="JPEG", quality=90)
        jpegs.append(buf.getvalue())
    res = {"config": os.path.relpath(f.config, ROOT), "source_hw": [H, W], "group_size": f.group, "warmup": f.warmup,
           "iters": f.iters, "device": torch.cuda.get_device_name(0)}
    # host decode
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < 2.0:
        inference.decode_image(jpegs[n % len(jpegs)])
        n += 1
    dt = time.perf_counter() - t0
    res["host_decode"] = {"images_per_s": n / dt, "ms_per_image": dt * 1e3 / n,
                          "mean_jpeg_kb": float(np.mean([len(j) for j in jpegs])) / 1024}
    print(json.dumps(res["host_decode"]), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        state = os.path.join(tmp, "model.ckpt.npz")
        np.savez(state, **{s.name: params.init_value(s, 1) for s in model_builder.variable_specs(cfg.model)})
        det = inference.Detector(f.config, state)
    res["resized_hw"] = list(det.resized_shape(H, W))
    dev, wall = _timed(torch, lambda: det.detect_images(pictures[:1]), f.warmup, f.iters)
    res["latency_b1"] = {"ms_per_image_events": dev, "ms_per_image_wall": wall}
    print(json.dumps(res["latency_b1"]), flush=True)
    dev, wall = _timed(torch, lambda: det.detect_images(pictures), f.warmup, f.iters)
    res["group"] = {"images_per_s_events": f.group * 1e3 / dev, "images_per_s_wall": f.group * 1e3 / wall,
                    "ms_per_call_events": dev}
    print(json.dumps(res["group"]), flush=True)
    dev, wall = _timed(torch, lambda: det.detect_encoded(jpegs), f.warmup, f.iters)
    res["encoded"] = {"images_per_s_events": f.group * 1e3 / dev, "images_per_s_wall": f.group * 1e3 / wall}
    print(json.dumps(res["encoded"]), flush=True)
    if f.out:
        with open(f.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
