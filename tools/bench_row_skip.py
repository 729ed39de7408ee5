"""Per-layer times of the closeness tower's backward GEMMs — the pointwise layers and the 3x3 layer on its Winograd plan
(block4 on 512 RoIs of 7x7 = 25 088 rows) — with the row-group flags of real bench batches: each shape timed with the flags honoured and ignored (mtlssl_conv2d_set_row_skip),
launches back to back between two events. On a tree without the flags (the parent of the row-skip change) the same
operands are timed through the plain calls, so the two trees' tables line up.

    python tools/bench_row_skip.py [--flags FILE] [--save-flags FILE] [--batches 4] [--reps 20] [--fraction F] [--only 1|3]

Without --flags the flags come from this tree's own bench model: configs/frcnn_resnet101_coco_mtl.config on the bench's
synthetic ring (seeds 1234 + 1000 i), one training step per batch, the flags each step derived from its loss scales.
--fraction F instead draws flags with that share of each image's 256 RoIs active, scattered (0.25 = the balanced sampler's
cap of 64 positives per image: the most a trained detector on real data can have active)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (mode, C, K): the filter gradients of conv3 / conv1 of units 2-3 / conv1 and shortcut of unit 1, the input gradients
# of conv3 and of conv1 of units 2-3 (the tower runs with need_input_grad=False: unit 1 sends nothing back); last field:
# filter size — the 3x3 conv2 of all three units, its filter gradient fed with the forward's kept input transform
SHAPES = [("wgrad", 512, 2048, 3, 1), ("wgrad", 2048, 512, 2, 1), ("wgrad", 1024, 512, 1, 1), ("wgrad", 1024, 2048, 1, 1),
          ("dgrad", 512, 2048, 3, 1), ("dgrad", 2048, 512, 2, 1), ("wgrad", 512, 512, 3, 3), ("dgrad", 512, 512, 3, 3)]


def bench_flags(n_batches):
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config")).read())
    dev = torch.device("cuda", 0)
    model = model_builder.build(cfg.model, True, dev, seed=0)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    B, K = int(cfg.train_config.batch_size), int(cfg.model.faster_rcnn.num_classes)
    out = []
    for i in range(n_batches):
        tr.step(tr.stage_batch(synthetic.make_batch(B, 600, 1024, K, seed=1234 + 1000 * i, device=dev)))
        torch.cuda.synchronize()
        out.append(tr._pd["_clo_active"].cpu().clone())
    del tr, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flags")
    ap.add_argument("--save-flags")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fraction", type=float)
    ap.add_argument("--only", type=int, default=0, help="1 / 3: only the 1x1 / only the 3x3 layers")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    has_skip = hasattr(ops, "set_row_skip")
    if a.fraction is not None:
        gf = torch.Generator().manual_seed(7)
        flags = []
        for _ in range(a.batches):
            f = torch.zeros(2, 256, dtype=torch.uint8)
            for b in range(2):
                f[b, torch.randperm(256, generator=gf)[:int(round(a.fraction * 256))]] = 1
            flags.append(f.view(-1))
    else:
        flags = torch.load(a.flags) if a.flags else bench_flags(a.batches)
    if a.save_flags:
        torch.save(flags, a.save_flags)
    active = [float(f.float().mean()) for f in flags]
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for mode, C, K, calls, ksize in SHAPES:
        if a.only and ksize != a.only:
            continue
        n = flags[0].numel()
        x = torch.randn(n, 7, 7, C, generator=gen, device="cuda")
        w = torch.randn(ksize, ksize, C, K, generator=gen, device="cuda") / (32.0 * ksize)
        dy0 = torch.randn(n, 7, 7, K, generator=gen, device="cuda")
        d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
        dw = torch.zeros_like(w)
        keep = {}
        if ksize == 3 and mode == "wgrad":
            ops.conv2d_fwd(d, x, w, keep_input_xf=keep)
        xf = keep.get(x.data_ptr())
        t = {}
        for on in ((1, 0) if has_skip else (None,)):
            if has_skip:
                ops.set_row_skip(on)
            per = []
            for f in flags:
                fl = f.cuda()
                dy = (dy0 * fl.view(-1, 1, 1, 1).float()).contiguous()
                kw = dict(active=fl) if has_skip else {}

                def run():
                    if mode == "wgrad":
                        ops.conv2d_wgrad(d, x, dy, dw, beta=0.0, input_xf=xf, **kw)
                    else:
                        ops.conv2d_dgrad(d, dy, w, None, x, ops.EPI_MASK, **kw)
                for _ in range(3):
                    run()
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.reps):
                    run()
                e.record()
                e.synchronize()
                per.append(1e3 * s.elapsed_time(e) / a.reps)
            t["skip_on_us" if on == 1 else "full_us"] = sum(per) / len(per)
        if has_skip:
            ops.set_row_skip(1)
        rows.append(dict(mode=mode, C=C, K=K, k=ksize, calls_per_step=calls, plan=ops.conv_plan_info(d, 1 if mode == "dgrad" else 2)["code"], **t))
        del x, w, dy0, dw, keep, xf
    print("| mode | filter | C | K | plan | calls/step | all rows us | flagged us | saved ms/step |\n|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        on = r.get("skip_on_us")
        print("| %s | %dx%d | %d | %d | %d | %d | %.1f | %s | %s |" % (
            r["mode"], r["k"], r["k"], r["C"], r["K"], r["plan"], r["calls_per_step"], r["full_us"], "%.1f" % on if on is not None else "-",
            "%.2f" % ((r["full_us"] - on) * r["calls_per_step"] / 1e3) if on is not None else "-"))
    print(json.dumps(dict(active_fraction_per_batch=active, rows=rows)))


if __name__ == "__main__":
    main()
