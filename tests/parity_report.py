"""Observed parity numbers of the GPU tests, printed in pytest's terminal summary (and appended to
gpurun_out/parity_report.txt when that directory exists) so that a drift from 1e-5 to 4e-3 cannot hide
behind a passing assert."""
import os

import numpy as np

LINES = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def add(line):
    LINES.append(line)
    d = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, "parity_report.txt"), "a") as f:
            f.write(line + "\n")


def gradients(tag, grads, ref, losses=None, ref_losses=None):
    """Per-variable relative L2 error of `grads` against `ref` ({name: ndarray}); records median / worst."""
    errs = []
    for name, g in grads.items():
        r = ref.get(name)
        if r is None:
            continue
        errs.append((float(np.linalg.norm((g - r).ravel()) / max(np.linalg.norm(r.ravel()), 1e-12)), name))
    errs.sort()
    l2 = np.array([e for e, _ in errs])
    line = "%s: %d variables, gradient rel-L2 median %.2e, p90 %.2e, worst %.2e (%s)" % (
        tag, len(l2), np.median(l2), np.percentile(l2, 90), l2[-1], errs[-1][1])
    if losses is not None:
        worst = max(abs(losses[k] - ref_losses[k]) / max(abs(ref_losses[k]), 1e-3) for k in ref_losses)
        line += "; loss rel err worst %.2e" % worst
    add(line)
    return l2


def dot_err(y, ref, scale):
    """max |y - ref| in units of 2^-24 * scale, where scale is the sum over the reduction of |a*b| (plus the magnitude of
    any addend the epilogue brings) — the natural unit of an fp32 dot product. `y` is the kernel's result (any device),
    `ref` / `scale` float64 CPU tensors of its shape. An output with scale 0 must be exactly 0 (e.g. the input pixels a
    strided convolution never reads)."""
    yd = y.double().cpu()
    live = scale > 0
    assert bool((yd[~live] == 0).all())
    return float(((yd - ref).abs()[live] / (scale[live] * 2.0 ** -24)).max())


def against_float64(tag, Oracle, hp, values, host_batch, seed, step, boxes, num, grads, cap=1e-3, outliers=12, worst=1e-2,
                    feat=None, d_feat=None, median_cap=3e-4, g32=None):
    """The gradient claim against the better yardstick: the same graph evaluated by the oracle in float64 AND in
    float32 on the DEVICE'S sampled boxes (`boxes` [B,N2,4] absolute, `num` [B]; forcing them takes the proposal chain
    and the crop knife edge at the image border — a sample at in_y = H-1 up to the last bit of a decoded box — out of
    the comparison). Asserted for the HIP path against float64:
      * every variable within `cap` (1e-3) relative L2, except at most `outliers` variables, none beyond `worst`;
      * those exceptions are what a single activation branch flip does: a pre-activation within an ulp of 0 (or 6)
        takes the other branch in one fp32 implementation, and one flipped element of a map moves every filter
        gradient behind it by ~1e-3 of its norm. The torch-CPU fp32 oracle shows the same class of outliers against
        float64 (reported next to the HIP path's). When the trunk's output map and its gradient are given (`feat`,
        `d_feat` = gradient masked by the last activation), the flips at that map are located and it is asserted that
        without those (at most 6; observed 1) elements the map's gradient agrees with float64 to 1e-4.
    Returns {name: (hip_vs_f64, fp32_oracle_vs_f64)}."""
    forced = dict(proposal_boxes=np.asarray(boxes), num_proposals=np.asarray(num))
    if g32 is None:          # (a caller that already holds the fp32 oracle's gradients on these boxes passes them in)
        _, g32, a32 = Oracle(hp, values).step(host_batch, seed=seed, step=step, forced=forced)
    _, g64, a64 = Oracle(hp, values, np.float64).step(host_batch, seed=seed, step=step, forced=forced)
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))
    out = {}
    for name, g in grads.items():
        if name in g64 and name in g32:
            out[name] = (rel(g, g64[name]), rel(g32[name], g64[name]))
    e_gpu = np.array([v[0] for v in out.values()])
    e_cpu = np.array([v[1] for v in out.values()])
    w_gpu = max(out, key=lambda n: out[n][0])
    w_cpu = max(out, key=lambda n: out[n][1])
    line = ("    vs float64 on the device's boxes (%s): HIP path worst %.2e (%s) median %.2e, %d of %d variables beyond %.0e; "
            "torch-CPU fp32 oracle worst %.2e (%s) median %.2e, %d beyond" % (
                tag, out[w_gpu][0], w_gpu.split("/", 1)[-1], np.median(e_gpu), int((e_gpu >= cap).sum()), len(e_gpu), cap,
                out[w_cpu][1], w_cpu.split("/", 1)[-1], np.median(e_cpu), int((e_cpu >= cap).sum())))
    if feat is not None and d_feat is not None:
        act6 = hp["arch"] == "mobilenet_v1"
        on = lambda F: (F > 0) & ((F < 6) if act6 else True)
        F64 = a64["features"]
        ref = a64["d_features"] * on(F64)
        flips = np.argwhere(on(np.asarray(feat)) != on(F64))
        keep = np.ones(ref.shape, bool)
        for f in flips:
            keep[tuple(f)] = False
        near = [float(min(abs(F64[tuple(f)]), abs(F64[tuple(f)] - 6.0) if act6 else np.inf)) for f in flips]
        e_all, e_wo = rel(np.asarray(d_feat), ref), rel(np.asarray(d_feat) * keep, ref * keep)
        line += ("; trunk output: %d activation flip(s) vs float64 (|pre-activation - threshold| <= %.1e of range %.1e), map "
                 "gradient rel err %.2e with them, %.2e without" % (len(flips), max(near) if near else 0.0, np.abs(F64).max(),
                                                                    e_all, e_wo))
        assert len(flips) <= 6 and all(v <= 1e-5 * np.abs(F64).max() for v in near), (tag, flips[:8], near[:8])
        assert e_wo < 1e-4, (tag, e_wo)
    add(line)
    assert np.median(e_gpu) < median_cap, (tag, np.median(e_gpu))
    assert int((e_gpu >= cap).sum()) <= outliers, (tag, sorted(((v[0], n) for n, v in out.items()), reverse=True)[:outliers + 2])
    assert e_gpu.max() < worst, (tag, w_gpu, e_gpu.max())
    return out


def oracle_on_device_rpn(Oracle, hp, values, host_batch, seed, step, pd, dtype=None, float_tol=1e-3):
    """The staged whole-step comparison every model-level test uses (a step is not one continuous function: the
    proposal chain — sort, greedy NMS, sampling — is discrete, and crop_and_resize switches from "interpolate" to
    "extrapolate with 0" at in_y = H - 1, where the last crop row of a box clipped to the image border sits up to the
    last bit of its decoded ymin):
      (1) the oracle evaluates trunk and RPN on its own (torch-CPU) and its RPN floats must agree with the device's to
          `float_tol` relative (asserted here) — the float claim up to the chain;
      (2) the oracle's chain runs ON THE DEVICE'S RPN FLOATS; identical inputs, so proposal counts, sampled boxes and
          detector matches must come out BIT FOR BIT (asserted here: no tolerance, no fallback);
      (3) everything downstream (crops, towers, heads, losses, gradients) is then compared by the caller with both
          sides looking at identical boxes.
    `pd` is the device's prediction_dict (faster_rcnn_meta_arch.py:593-601, 693-699). -> (losses, grads, aux)."""
    enc = pd["rpn_box_encodings"].cpu().numpy()
    obj = pd["rpn_objectness_predictions_with_background"].cpu().numpy()
    ora = Oracle(hp, values) if dtype is None else Oracle(hp, values, dtype)
    ref, rgrads, aux = ora.step(host_batch, seed=seed, step=step, forced=dict(rpn_box_encodings=enc, rpn_objectness=obj))
    for mine, theirs in ((enc, aux["rpn_box_encodings"]), (obj, aux["rpn_objectness"])):
        assert float(np.abs(mine - theirs).max()) <= float_tol * float(np.abs(theirs).max()), \
            (float(np.abs(mine - theirs).max()), float(np.abs(theirs).max()))
    if "proposal_boxes" in pd:
        np.testing.assert_array_equal(pd["num_proposals"].cpu().numpy(), aux["num_proposals"])
        np.testing.assert_array_equal(pd["proposal_boxes"].cpu().numpy(), aux["proposal_boxes"])
        if "_det_targets" in pd and "det_match" in aux:
            np.testing.assert_array_equal(pd["_det_targets"]["match"].cpu().numpy(), aux["det_match"])
    return ref, rgrads, aux
