"""What the float32 matmul precision levels cost and buy on one MI355X (reported, not gated; not part of bench.py).

    python tools/matmul_precision_rate.py --out profiles/matmul_precision_rate.json

configs/frcnn_resnet101_coco_mtl.config (configs[1]) at B = 2 on a ring of synthetic device batches (600x1024). ONE process,
one model: the four levels of ops.FP32_ENGINES take turns (highest, split, high, medium; three passes), each turn
10 warm-up + 30 timed steps between device synchronises, so clock drift and other tenants of the host hit every level
alike; the spread over the three passes is reported beside the median. One JSON document:
  levels.<name>.ms_per_step            median of the passes, and every pass (ms_per_step_passes)
  levels.<name>.launches_per_step      ops.engine_launches over a timed window / steps: native, six, three, one
  levels.<name>.loss_minus_highest     each loss term of ONE forward + backward on the same weights and the same batch,
                                       minus the same term under `highest` (loss_highest holds those)
  levels.<name>.grad_rel_distance      per-variable |g - g_highest|_2 / |g_highest|_2 of that step: median, worst (+ its name)
The accuracy step runs before the timed passes, on the initial weights. A level changes the RPN's floats, so the proposal
chain may sample other boxes: the distances are whole-model measurements, not kernel bounds (tests/matmul_precision holds those)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config")


def accuracy_step(tr, batch, names):
    """One forward + backward per level on the same state and batch -> {level: (losses, per-variable gradients)}."""
    import torch
    from mtl_ssl_amd import ops
    out = {}
    for name in names:
        ops.set_float32_matmul_precision(name)
        losses = tr.forward_backward(batch)
        torch.cuda.synchronize()
        ps = tr.ps
        out[name] = ({k: float(v.item()) for k, v in losses.items()},
                     {s.name: ps.grad(s.name).detach().double().clone() for s in ps.trainable_specs})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=CONFIG)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import __graft_entry__ as ge
    ge.build()
    if not torch.cuda.is_available():
        raise SystemExit("matmul_precision_rate needs a GPU: a CPU run says nothing about these times")
    from mtl_ssl_amd import config, model_builder, ops, synthetic, trainer
    dev = torch.device("cuda", 0)
    cfg = config.parse_pipeline_config(open(a.config).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    names = list(ops.FP32_ENGINES)
    before = ops.get_float32_matmul_precision()
    model = model_builder.build(cfg.model, True, dev, seed=0)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    ring = [tr.stage_batch(synthetic.make_batch(a.batch, a.height, a.width, K, seed=1234 + 1000 * i, device=dev))
            for i in range(4)]
    levels = {n: {"mode": ops.FP32_ENGINES[n], "ms_per_step_passes": []} for n in names}
    try:
        acc = accuracy_step(tr, ring[0], names)
        l0, g0 = acc["highest"]
        for n in names:
            ln, gn = acc[n]
            dist = {v: float((gn[v] - g0[v]).norm() / g0[v].norm()) for v in g0 if float(g0[v].norm()) > 0}
            worst = max(dist, key=dist.get)
            levels[n]["loss_minus_highest"] = {k: ln[k] - l0[k] for k in l0}
            levels[n]["grad_rel_distance"] = {"median": float(np.median(list(dist.values()))), "worst": dist[worst],
                                              "worst_variable": worst, "variables": len(dist)}
        del acc, g0
        for p in range(a.passes):
            for n in names:
                ops.set_float32_matmul_precision(n)
                for i in range(a.warmup):
                    tr.step(ring[i % 4])
                torch.cuda.synchronize()
                ops.engine_launches(reset=True)
                t0 = time.perf_counter()
                for i in range(a.steps):
                    losses = tr.step(ring[(a.warmup + i) % 4])
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / a.steps
                counts = ops.engine_launches(reset=True)
                levels[n]["ms_per_step_passes"].append(1e3 * dt)
                levels[n]["launches_per_step"] = {k: v / a.steps for k, v in counts.items()}
                levels[n]["total_loss_last_step"] = float(sum(v.item() for v in losses.values()))
                print(json.dumps({"pass": p, "level": n, "ms_per_step": 1e3 * dt, "launches_per_step": levels[n]["launches_per_step"]}),
                      flush=True)
    finally:
        ops.set_float32_matmul_precision(before)
    for n in names:
        ms = levels[n]["ms_per_step_passes"]
        levels[n]["ms_per_step"] = float(np.median(ms))
        levels[n]["ms_per_step_spread"] = max(ms) - min(ms)
    res = {"config": os.path.relpath(a.config, ROOT), "device": torch.cuda.get_device_name(0), "per_gpu_batch": a.batch,
           "image": "%dx%d" % (a.width, a.height), "steps": a.steps, "warmup": a.warmup, "passes": a.passes, "runs": 1,
           "order": names, "loss_highest": l0, "levels": levels}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
