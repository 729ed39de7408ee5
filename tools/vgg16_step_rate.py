"""Step rate of the Faster R-CNN VGG-16 configuration on one MI355X (reported, not gated; not part of bench.py).

    python tools/vgg16_step_rate.py --out profiles/vgg16_step_rate.json

configs/vgg16/frcnn_vgg16_voc_mtl.config at B = 2 on a ring of synthetic device batches (600x1024), 10 warm-up and 30 timed
steps, one run. One JSON document:
  ms_per_step, images_per_sec, executed_mfma_tflop_per_step (from the descriptors, ops.FlopAccount)
  trunk_plans       the resolver's plan per trunk layer and mode (forward / input gradient / filter gradient)
  freeze_layer      ms/step of the same configuration with freeze_layer '' against 'conv2' (the configuration's own)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "configs", "vgg16", "frcnn_vgg16_voc_mtl.config")
MODES = ("forward", "dgrad", "wgrad")


def run(text, B, H, W, steps, warmup, dev, plans=False):
    import torch
    from mtl_ssl_amd import config, model_builder, ops, synthetic, trainer
    cfg = config.parse_pipeline_config(text)
    K = int(cfg.model.faster_rcnn.num_classes)
    torch.cuda.reset_peak_memory_stats()
    model = model_builder.build(cfg.model, True, dev, seed=0)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    ring = [tr.stage_batch(synthetic.make_batch(B, H, W, K, seed=1234 + 1000 * i, device=dev)) for i in range(4)]
    for i in range(warmup):
        tr.step(ring[i % 4])
    torch.cuda.synchronize()
    ops.ACCOUNT = ops.FlopAccount()
    t0 = time.perf_counter()
    for i in range(steps):
        losses = tr.step(ring[(warmup + i) % 4])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    account, ops.ACCOUNT = ops.ACCOUNT, None
    out = {"freeze_layer": str(cfg.model.faster_rcnn.feature_extractor.freeze_layer), "ms_per_step": 1e3 * dt,
           "images_per_sec": B / dt, "steps": steps, "warmup": warmup,
           "executed_mfma_tflop_per_step": sum(r[1] for r in account.rows.values()) * 2.0 / steps / 1e12,
           "executed_by_class": {k: {"calls_per_step": r[0] / steps, "mfma_tflop_per_step": r[1] * 2.0 / steps / 1e12}
                                 for k, r in sorted(account.rows.items())},
           "total_loss": float(sum(v.item() for v in losses.values())),
           "peak_memory_gb": torch.cuda.max_memory_allocated() / 2.0 ** 30}
    if plans:
        rows, shape = [], (B, H, W, 3)
        fe = model._feature_extractor
        for g, convs in enumerate(fe.groups):
            for l in convs:
                d = l.desc(shape)
                row = {"layer": l.scope.split("/")[-1], "input": list(shape), "cout": l.cout, "trainable": bool(l.trainable)}
                for mode, name in enumerate(MODES):
                    info = ops.conv_plan_info(d, mode)
                    row[name] = {k: info[k] for k in ("family", "code", "BM", "BN", "nsplit", "dispatches")}
                rows.append(row)
                shape = (B, shape[1], shape[2], l.cout)
            if g < len(fe.groups) - 1:
                shape = (B, shape[1] // 2, shape[2] // 2, shape[3])
        out["trunk_plans"] = rows
    del model, tr, ring
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=CONFIG)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        raise SystemExit("vgg16_step_rate needs a GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda", 0)
    text = open(a.config).read()
    own = "freeze_layer: 'conv2'"
    if text.count(own) != 1:
        raise SystemExit("%s: expected exactly one %s" % (a.config, own))
    main_run = run(text, a.batch, a.height, a.width, a.steps, a.warmup, dev, plans=True)
    print(json.dumps({k: v for k, v in main_run.items() if k != "trunk_plans"}), flush=True)
    all_train = run(text.replace(own, "freeze_layer: ''"), a.batch, a.height, a.width, a.steps, a.warmup, dev)
    res = {"config": os.path.relpath(a.config, ROOT), "device": torch.cuda.get_device_name(0), "per_gpu_batch": a.batch,
           "image": "%dx%d" % (a.width, a.height), "runs": 1}
    res.update(main_run)
    res["freeze_layer_ms_per_step"] = {"conv2": main_run["ms_per_step"], "": all_train["ms_per_step"]}
    res["freeze_layer_all_trainable"] = {k: all_train[k] for k in ("ms_per_step", "executed_mfma_tflop_per_step",
                                                                   "peak_memory_gb")}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
