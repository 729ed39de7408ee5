"""What batch-statistics BatchNorm in the heads costs on one MI355X.

    python tools/batch_norm_cost.py [--out profiles/batch_norm_cost.json] [--steps 30] [--passes 3]

1. Kernel time per call, alone: mtlssl_batch_norm_train_fwd (ReLU epilogue, moving averages updated) and
   mtlssl_batch_norm_train_bwd (ReLU mask, gamma / beta gradients) at 4864 x 512 (the RPN conv of the 2-image
   600 x 1024 configuration), 512 x 1024 and 512 x 4096 (FC layers over 512 RoIs). Device events around `--reps` calls
   after a warm-up, the median of five such windows; bytes = the passes over x / y / dy / dx the kernel makes.
2. ms / step of configs/batch_norm/smoke_resnet50_bn_mtl.config against the same text without its two `batch_norm`
   blocks: both trainers live in one process, timed alternately, `--passes` passes of `--steps` steps each, host clock
   around steps that end in a device synchronise. A 160 x 224 smoke model: the figure is the normalisers' launches
   against a step of small kernels, not a full-size step.

There is no pass / fail threshold. Needs a GPU; fails without one."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4864, 512), (512, 1024), (512, 4096)]


def kernel_times(reps):
    import torch
    from mtl_ssl_amd import ops
    out = []
    for rows, C in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(rows + C)
        x = torch.randn((rows, C), device="cuda", generator=g)
        dy = torch.randn((rows, C), device="cuda", generator=g)
        gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        mm, mv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        y, sm, si = ops.batch_norm_train_fwd(x, gamma, beta, 1e-3, ops.EPI_RELU, mm, mv, 1e-3)
        dx = torch.empty_like(x)

        def fwd():
            ops.batch_norm_train_fwd(x, gamma, beta, 1e-3, ops.EPI_RELU, mm, mv, 1e-3, y=y, save_mean=sm, save_inv_std=si)

        def bwd():
            ops.batch_norm_train_bwd(x, dy, gamma, sm, si, dg, db, y=y, mask_epilogue=ops.EPI_MASK, dx=dx)

        row = {"rows": rows, "C": C}
        for name, fn, passes in (("fwd", fwd, 4), ("bwd", bwd, 7)):      # fwd: 3 reads of x + y; bwd: 2 x (x, dy, y) + dx
            for _ in range(10):
                fn()
            windows = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                windows.append(a.elapsed_time(b) * 1e3 / reps)
            us = statistics.median(windows)
            row[name + "_us"] = round(us, 2)
            row[name + "_us_windows"] = [round(w, 2) for w in windows]
            row[name + "_bytes_touched"] = passes * rows * C * 4
            row[name + "_GBps_touched"] = round(passes * rows * C * 4 / us / 1e3, 1)
        out.append(row)
    return out


def step_times(steps, passes):
    import re
    import torch
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    text = open(os.path.join(ROOT, "configs", "batch_norm", "smoke_resnet50_bn_mtl.config")).read()
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    plain, n = re.subn(r"batch_norm \{[^}]*\}", "", text)
    assert n == 2, n
    trainers = {}
    for name, t in (("batch_norm", text), ("without", plain)):
        cfg = config.parse_pipeline_config(t)
        model = model_builder.build(cfg.model, True, "cuda", seed=1)
        trainers[name] = trainer.Trainer(model, cfg.train_config, 1)
    batch = {k: trainers[k].stage_batch(synthetic.make_batch(2, 160, 224, 5, seed=5, device="cuda", max_gt=4, num_windows=6))
             for k in trainers}
    for k, tr in trainers.items():
        for _ in range(10):
            tr.step(batch[k])
    torch.cuda.synchronize()
    out = {k: [] for k in trainers}
    for _ in range(passes):
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step(batch[k])
            torch.cuda.synchronize()
            out[k].append(round((time.perf_counter() - t0) * 1e3 / steps, 4))
    return {"config": "configs/batch_norm/smoke_resnet50_bn_mtl.config", "image": [160, 224], "batch": 2,
            "steps_per_pass": steps, "ms_per_step": out,
            "median_ms_per_step": {k: statistics.median(v) for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_norm_cost.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available(), "tools/batch_norm_cost.py measures on a GPU"
    result = {"device": torch.cuda.get_device_name(0), "kernels": kernel_times(args.reps),
              "step": step_times(args.steps, args.passes)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
