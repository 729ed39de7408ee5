"""GPU: the small kernels of the training step (loss weights, class-selected box loss, the two loss kernels at their
call sites' shapes, refine-input assembly, activation gradients, the shipped SGD update with its BatchNorm /
residual-scale folds), each against a float64 NumPy restatement of the reference's formula.

Tolerances follow from the arithmetic (eps = 2^-23, the fp32 machine epsilon):
  * data movement and comparisons are bit-exact;
  * a fixed short fp32 sequence of r roundings is within r * eps/2 relative of float64 (bounds stated per op);
  * a reduction is within c * depth * eps * sum|terms| of float64, with `depth` the kernel's own summation depth
    (the longest chain of additions any one term passes through), so a dropped term or a wrong count fails it."""
import os
import types

import numpy as np
import pytest
import torch

from tests.f64_check import EPS, TINY, bits, dev, host, within

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


def _configs1():
    from mtl_ssl_amd import config
    return config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "frcnn_resnet101_coco_mtl.config")).read())


# ---------------------------------------------------------------------------------------------------- loss weights
# RPN sizes: configs[1]'s anchors inside the image / all anchors of its 38x64 grid x 12, MobileNet's 38x50x12
@pytest.mark.parametrize("n", [14453, 29184, 38 * 50 * 12, 1000])
def test_rpn_loss_scales_against_float64(ops, n):
    rs = np.random.RandomState(11)
    B = 3
    sampled = (rs.rand(B, n) < 256.0 / n).astype(f32)
    sampled[1] = 0.0                                            # an image with nothing sampled: the inv = 0 path
    sampled[2, -1] = 1.0                                        # the last (tail) anchor counts
    reg_w = rs.rand(B, n).astype(f32)
    loc_coef, obj_coef = 2.0 / B, 1.0 / B
    ls, os_ = ops.rpn_loss_scales(dev(sampled), dev(reg_w), loc_coef, obj_coef)
    # faster_rcnn_meta_arch.py:1644-1659: normalizer = reduce_sum(sampled, axis=1); the loss is
    # reduce_sum(loss * weights) / normalizer, i.e. per-anchor weight sampled * reg_w * coef / normalizer. The reference
    # divides 0 by 0 for an image with nothing sampled; the kernel gives that image zero weight (k_rpn_loss_scales).
    S = sampled.astype(np.float64).sum(1, keepdims=True)
    inv = np.where(S > 0, 1.0 / np.maximum(S, 1.0), 0.0)
    loc_ref = sampled * reg_w.astype(np.float64) * f32(loc_coef) * inv
    obj_ref = sampled * np.float64(f32(obj_coef)) * inv
    # S is a sum of 0/1 values below 2^24: exact in any order. Then (s * w) * coef * inv and s * coef * inv with a
    # rounded reciprocal: four roundings at most, bound 2 eps relative.
    within(host(ls), loc_ref, 2 * EPS * np.abs(loc_ref), "rpn loc scale")
    within(host(os_), obj_ref, 2 * EPS * np.abs(obj_ref), "rpn obj scale")
    assert not host(ls)[1].any() and not host(os_)[1].any()
    assert (host(os_)[sampled == 0] == 0).all()


@pytest.mark.parametrize("k1", [2, 21, 91])
@pytest.mark.parametrize("n2", [1, 16, 64, 255, 256, 257, 300, 512])
def test_detector_loss_scales_against_float64(ops, n2, k1):
    rs = np.random.RandomState(1000 * n2 + k1)
    B = 4
    num = np.array([0, 1, max(n2 - 1, 0), n2], np.int32)     # per image: none, one, all but one, all
    cls_w = np.where(rs.rand(B, n2) < 0.8, 1.0, rs.rand(B, n2)).astype(f32)
    reg_w = np.where(rs.rand(B, n2) < 0.3, 1.0, 0.0).astype(f32)
    reg_w[2] *= rs.rand(n2).astype(f32)                         # fractional weights in one image
    reg_w[3, -1] = 1.0                                          # the tail row counts in the closeness normaliser
    clo_t = (rs.rand(B * n2, k1) * (rs.rand(B * n2, k1) < 0.5)).astype(f32)
    clo_t[::5] = 0.0                                            # rows without any closeness target
    coefs = (1.0, 2.0, 0.3)
    for with_clo in (True, False):
        cs, ls, qs = ops.detector_loss_scales(dev(cls_w), dev(reg_w), dev(num), dev(clo_t) if with_clo else None, *coefs)
        # faster_rcnn_meta_arch.py:1715-1725: normalizer = max(num_proposals, 1) * batch_size; losses / normalizer,
        # summed over the non-padding rows only (boolean_mask(paddings_indicator), :1736-1741)
        pad = (np.arange(n2)[None, :] < num[:, None]).astype(np.float64)
        norm = np.maximum(num, 1)[:, None].astype(np.float64) * B
        cls_ref = cls_w * pad / norm * f32(coefs[0])
        loc_ref = reg_w * pad / norm * f32(coefs[1])
        # w * pad / normalizer * coef with an exact integer normalizer: two roundings, bound eps relative
        within(host(cs), cls_ref, EPS * np.abs(cls_ref), "detector cls scale")
        within(host(ls), loc_ref, EPS * np.abs(loc_ref), "detector loc scale")
        assert not host(cs)[pad == 0].any() and not host(ls)[pad == 0].any(), "padding rows must weigh exactly 0"
        if not with_clo:
            assert qs is None
            continue
        # :1774-1789: normalizer_reg = max(1, sum over ALL max_num_proposals rows of reg_w); closeness loss of a row
        # = loss * reg_w / normalizer_reg * sum(closeness targets without background); no padding mask there
        R = np.maximum(1.0, reg_w.astype(np.float64).sum(1, keepdims=True))
        st = clo_t.astype(np.float64)[:, 1:].sum(1).reshape(B, n2)
        clo_ref = reg_w / R * st * f32(coefs[2])
        # every term is >= 0, so the bound is relative: sum of reg_w (256-strided lanes, 6 wave levels, 3 adds
        # across the waves), sum of k1-1 targets (sequential), then three roundings
        depth_r = -(-n2 // 256) + 6 + 3
        within(host(qs), clo_ref, EPS * (depth_r + (k1 - 1) + 3) * np.abs(clo_ref), "closeness scale")
        assert not host(qs)[reg_w == 0].any()


# --------------------------------------------------------------------------------------------- smooth L1 family
def _smooth_l1_terms(d, sigma):
    """core/losses.py:183-192 in float64. The threshold is the fp32 constant the reference compares with
    (1./sigma_sq, a Python float converted to the fp32 tensor's type)."""
    inv = np.float64(f32(1.0 / (sigma * sigma)))
    ad = np.abs(d)
    quad = ad < inv
    term = np.where(quad, 0.5 * ad * ad * sigma * sigma, ad - 0.5 * inv)
    grad = np.where(quad, d * sigma * sigma, np.sign(d))
    return term, grad, quad


def _smooth_l1_fp32(d, sigma):
    """The same formula evaluated in fp32 in the reference's order, term by term (every step one correctly rounded
    fp32 operation, so the branch taken shows in the bits)."""
    s2 = f32(sigma) * f32(sigma)
    inv = f32(1.0) / s2
    ad = np.abs(d.astype(f32))
    quad = ad < inv
    term = np.where(quad, f32(0.5) * ad * ad * s2, ad - f32(0.5) * inv).astype(f32)
    grad = np.where(quad, d.astype(f32) * s2, np.sign(d).astype(f32)).astype(f32)
    return term, grad


def _seq_sum(t):
    acc = np.zeros(t.shape[0], f32)
    for j in range(t.shape[1]):                                    # the kernel's order, in fp32
        acc = (acc + t[:, j]).astype(f32)
    return acc


@pytest.mark.parametrize("sigma", [1.0, 3.0])
@pytest.mark.parametrize("K", [5, 20, 90])
def test_box_select_smooth_l1_against_float64(ops, K, sigma):
    from mtl_ssl_amd.lib import ptr
    rs = np.random.RandomState(7 * K + int(sigma))
    rows = 517                                                     # not a multiple of the 256-thread block
    cls = rs.randint(0, K + 1, rows)                              # 0 = background
    cls[:40] = 0
    cls_t = np.zeros((rows, K + 1), f32)
    cls_t[np.arange(rows), cls] = 1.0
    cls_t[40:48] = 0.0                                             # rows without any target class
    cls[40:48] = 0
    refined = rs.randn(rows, K, 4).astype(f32)
    reg_t = (rs.randn(rows, 4) * 0.5).astype(f32)
    w = rs.rand(rows).astype(f32)
    inv = f32(1.0) / (f32(sigma) * f32(sigma))
    edge = np.array([inv, np.nextafter(inv, f32(0)), -np.nextafter(inv, f32(np.inf)), f32(0.0)], f32)
    # rows 100..107: |d| exactly at the threshold and one ulp to either side (tf.less, core/losses.py:188), d == 0
    for r in range(100, 108):
        c = 1 + (r % K)
        cls_t[r] = 0.0
        cls_t[r, c] = 1.0
        cls[r] = c
        reg_t[r] = 0.0
        refined[r, c - 1] = np.roll(edge, r)
        w[r] = 1.0
    for r in range(20, 24):                                        # background rows at the threshold: prediction 0
        reg_t[r] = -np.roll(edge, r)
    # faster_rcnn_meta_arch.py:1735-1749: pad a zero background slot, select the slot of the target class, smooth L1
    # against the regression target with the row's weight
    padded = np.concatenate([np.zeros((rows, 1, 4)), refined.astype(np.float64)], 1)
    pred = padded[np.arange(rows), cls]
    d = pred - reg_t
    term, grad, _ = _smooth_l1_terms(d, sigma)
    loss_ref = term.sum(1) * w
    dref = np.zeros((rows, K + 1, 4))
    dref[np.arange(rows), cls] = grad * w[:, None]
    dref = dref[:, 1:]
    # the gradient buffer starts as NaN: the launcher's memset must cover every element the kernel does not write
    rd, td, cd, wd = dev(refined), dev(reg_t), dev(cls_t), dev(w)
    rl = torch.empty(rows, device="cuda")
    dr = torch.full_like(rd, float("nan"))
    ops.lib().box_select_smooth_l1(ptr(rd), ptr(cd), ptr(td), ptr(wd), rows, K, float(sigma), ptr(rl), ptr(dr),
                                   ops._stream())
    got_l, got_d = host(rl), host(dr)
    # four terms of at most three roundings each, four additions, the weight: bound 8 eps of the row's |terms|
    within(got_l, loss_ref, 8 * EPS * w * np.abs(term).sum(1) + 0.0, "box loss")
    # d * sigma^2 * w (the difference itself rounded once): bound 2 eps relative; sign(d) * w exact
    within(got_d, dref, 2 * EPS * np.abs(dref), "box loss gradient")
    sel = np.zeros((rows, K + 1), bool)
    sel[np.arange(rows), cls] = True
    sel = sel[:, 1:]
    assert not np.isnan(got_d).any()
    assert (got_d[~sel] == 0).all(), "only the target class's 4 encodings of a positive row receive a gradient"
    assert (got_d[cls == 0] == 0).all()
    # the threshold rows: the branch taken must be the reference's, bit for bit
    t32, g32 = _smooth_l1_fp32(d[100:108].astype(f32), sigma)
    bits(got_l[100:108], _seq_sum(t32), "threshold rows: loss")
    bits(got_d[np.arange(100, 108), cls[100:108] - 1], g32, "threshold rows: gradient")
    t32, _ = _smooth_l1_fp32(d[20:24].astype(f32), sigma)
    bits(got_l[20:24], _seq_sum(t32) * w[20:24], "background threshold rows: loss")
    # want_grad=False: the same losses, no gradient buffer
    rl2, dr2 = ops.box_select_smooth_l1(rd, cd, td, wd, sigma, want_grad=False)
    assert dr2 is None
    bits(host(rl2), got_l, "want_grad=False")
    rl3, dr3 = ops.box_select_smooth_l1(rd, cd, td, wd, sigma)
    bits(host(dr3), got_d, "wrapper vs NaN-filled buffer")


def test_rpn_smooth_l1_and_objectness_at_call_site_shapes(ops):
    """frcnn.py:779-783 at configs[1]'s size: 2 x 14 453 anchors, sigma 3, the onehot2 objectness targets."""
    rs = np.random.RandomState(3)
    rows = 2 * 14453
    pred = rs.randn(rows, 4).astype(f32)
    tgt = (rs.randn(rows, 4) * 0.3).astype(f32)
    wt = np.where(rs.rand(rows) < 0.05, rs.rand(rows), 0.0).astype(f32)
    rl, dp = ops.smooth_l1(dev(pred), dev(tgt), dev(wt), 3.0)
    term, grad, _ = _smooth_l1_terms(pred.astype(np.float64) - tgt, 3.0)
    within(host(rl), term.sum(1) * wt, 8 * EPS * wt * np.abs(term).sum(1), "rpn smooth l1")
    gref = grad * wt[:, None]
    within(host(dp), gref, 2 * EPS * np.abs(gref), "rpn smooth l1 gradient")
    rl2, dp2 = ops.smooth_l1(dev(pred), dev(tgt), dev(wt), 3.0, want_grad=False)
    assert dp2 is None
    bits(host(rl2), host(rl), "smooth_l1 want_grad=False")
    # objectness: onehot2 of the {0, 1} class targets is data movement
    cls_t = (rs.rand(rows) < 0.3).astype(f32)
    oh = ops.onehot2(dev(cls_t))
    ref_oh = np.stack([cls_t == 0, cls_t == 1], -1).astype(f32)
    bits(host(oh), ref_oh, "onehot2")
    logits = (rs.randn(rows, 2) * 4).astype(f32)
    rl, dl = ops.softmax_ce(dev(logits), oh, dev(wt))
    _check_softmax_ce(host(rl), host(dl), logits, ref_oh, wt, 0, 2, "rpn objectness")


def _softmax_ce_ref(logits, targets, w, col0, C):
    """core/losses.py WeightedSoftmaxClassificationLoss (softmax_cross_entropy_with_logits * weights) in float64:
    loss = w * sum_c t_c (lse - x_c), dloss/dx = w * (softmax(x) * sum(t) - t)."""
    x = logits[:, col0:col0 + C].astype(np.float64)
    t = targets[:, col0:col0 + C].astype(np.float64)
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    se = e.sum(1, keepdims=True)
    lse = np.log(se)
    st = t.sum(1, keepdims=True)
    w = w.astype(np.float64)[:, None]
    loss = (w * (st * lse - (t * (x - m)).sum(1, keepdims=True)))[:, 0]
    p = e / se
    grad = w * (p * st - t)
    return loss, grad, x - m, t, lse, p, st


def _check_softmax_ce(got_l, got_d, logits, targets, w, col0, C, what):
    loss, grad, xm, t, lse, p, st = _softmax_ce_ref(logits, targets, w, col0, C)
    # one wavefront per row: each lane sums ceil(C/64) columns, then 6 butterfly levels; exp / log add a few ulps
    depth = -(-C // 64) + 6 + 4
    aw = np.abs(w.astype(np.float64))
    tol_l = 2 * depth * EPS * aw * ((np.abs(t) * (1 + lse)).sum(1) + np.abs(t * xm).sum(1))
    within(got_l, loss, tol_l + aw * TINY, what + ": row loss")
    if got_d is None:
        return
    tol_g = 2 * depth * EPS * aw[:, None] * (p * st + np.abs(t)) + aw[:, None] * st * TINY
    within(got_d[:, col0:col0 + C], grad, tol_g, what + ": gradient")
    assert not got_d[:, :col0].any() and not got_d[:, col0 + C:].any(), what + ": columns outside [col0, col0+C)"


def _spread_logits(rs, rows, C):
    x = (rs.randn(rows, C) * 3).astype(f32)
    x[::7] = rs.uniform(-300, 300, (len(x[::7]), C)).astype(f32)   # a non-max-subtracted exp overflows here
    return x


def test_detector_and_closeness_softmax_ce_at_call_site_shapes(ops):
    """frcnn.py:806-838 at configs[1]'s sizes: 512 rows x 91 classes with the row scale; closeness over columns 1..90
    of a 91-wide row. One-hot, soft and all-zero targets, logits over +-300, 4 rows per block with a ragged tail."""
    cfg = _configs1()
    K1 = int(cfg.model.faster_rcnn.num_classes) + 1
    rows = 2 * int(cfg.model.faster_rcnn.second_stage_batch_size)
    rs = np.random.RandomState(5)
    for n in (rows, rows - 1, 3):                                 # 512, then ragged against the 4-row block
        logits = _spread_logits(rs, n, K1)
        t = np.zeros((n, K1), f32)
        t[np.arange(n), rs.randint(0, K1, n)] = 1.0
        t[1::5] = (rs.rand(len(t[1::5]), K1) * (rs.rand(len(t[1::5]), K1) < 0.2)).astype(f32)   # soft targets
        t[2::9] = 0.0                                              # targets summing to 0
        w = rs.rand(n).astype(f32)
        rl, dl = ops.softmax_ce(dev(logits), dev(t), dev(w))
        gl, gd = host(rl), host(dl)
        _check_softmax_ce(gl, gd, logits, t, w, 0, K1, "detector %d rows" % n)
        assert (gl[2::9] == 0).all() and (gd[2::9] == 0).all(), "a row without targets has no loss and no gradient"
        rl2, dl2 = ops.softmax_ce(dev(logits), dev(t), dev(w), want_grad=False)
        assert dl2 is None
        bits(host(rl2), gl, "softmax_ce want_grad=False")
        # closeness: softmax over columns 1.. of the 91-wide row (faster_rcnn_meta_arch.py:1777-1778)
        rl, dl = ops.softmax_ce(dev(logits), dev(t), dev(w), col0=1)
        _check_softmax_ce(host(rl), host(dl), logits, t, w, 1, K1 - 1, "closeness %d rows" % n)
        assert not host(dl)[:, 0].any(), "closeness: column 0 of dlogits stays zero"


def test_edgemask_targets_and_loss_at_call_site_shapes(ops):
    """frcnn.py:843-850: edge-mask targets from the synthetic batch's [2, mask, mask] labels, the softmax loss over
    B * mask * mask rows and its reduce_sum."""
    from mtl_ssl_amd import synthetic
    cfg = _configs1()
    r = cfg.model.faster_rcnn.image_resizer.keep_aspect_ratio_resizer
    K = int(cfg.model.faster_rcnn.num_classes)
    B = 2
    batch = synthetic.make_batch(B, int(r.min_dimension), int(r.max_dimension), K, seed=9, device="cpu", max_gt=6,
                                 num_windows=4)
    em = np.stack(batch["groundtruth_edgemask"]).astype(f32)      # [B, 2, mh, mw]
    _, _, mh, mw = em.shape
    coef = float(cfg.model.mtl.edgemask_loss_weight) / (B * mh * mw)
    tgt, sc = ops.edgemask_targets(dev(em), coef)
    fg, wgt = em[:, 0], em[:, 1]
    # faster_rcnn_meta_arch.py:1862-1868: targets (1 - fg, fg), per-pixel weight * coef: one fp32 operation each
    bits(host(tgt), np.stack([f32(1) - fg, fg], -1), "edgemask targets")
    bits(host(sc), wgt * f32(coef), "edgemask row scale")
    rows = B * mh * mw
    rs = np.random.RandomState(2)
    logits = (rs.randn(rows, 2) * 5).astype(f32)
    rl, dl = ops.softmax_ce(dev(logits), tgt.view(rows, 2), sc.view(-1))
    tflat, sflat = host(tgt).reshape(rows, 2), host(sc).reshape(rows)
    _check_softmax_ce(host(rl), host(dl), logits, tflat, sflat, 0, 2, "edgemask")
    _check_reduce_sum(ops, host(rl), 1.0, "edgemask loss")


def _check_reduce_sum(ops, x, scale, what):
    out = host(ops.reduce_sum(dev(x), scale))[0]
    ref = x.astype(np.float64).sum() * np.float64(f32(scale))
    # 1024 threads: each sums ceil(n/1024) elements in order, then a 10-level tree, then the scale
    depth = -(-len(x) // 1024) + 10 + 1
    within(out, ref, depth * EPS * np.abs(x.astype(np.float64)).sum() * abs(scale), what)


def test_reduce_sum_against_float64(ops):
    rs = np.random.RandomState(8)
    mask = 64                                                      # labels.edgemask's mask_size (synthetic batch)
    # the largest edge-mask loss: R-FCN's per-GPU batch of 4 (BASELINE configs[2]) x mask x mask rows; the RPN's
    # 2 x 29 184 anchors
    for n in (1, 1023, 1024, 1025, 29184, 4 * mask * mask, 2 * 29184):
        x = rs.randn(n).astype(f32)
        x[-1] = 1000.0                                             # a dropped tail element cannot hide in the bound
        if n > 1024:
            x[1024] = -700.0                                       # nor the first element of a lane's second pass
        _check_reduce_sum(ops, x, 0.37, "reduce_sum n=%d" % n)
        _check_reduce_sum(ops, x, 1.0, "reduce_sum n=%d scale 1" % n)


# ------------------------------------------------------------------------------------------------ refine glue
@pytest.mark.parametrize("k1", [2, 21, 91])
@pytest.mark.parametrize("n2", [1, 7, 8, 9, 300, 512])
def test_refine_concat_against_float64(ops, n2, k1):
    from mtl_ssl_amd import frcnn
    E = frcnn.FasterRCNNMetaArch.N_EXPAND
    rs = np.random.RandomState(100 * n2 + k1)
    for B in (1, 2):
        cls = rs.randn(B * n2, k1).astype(f32)
        win = rs.randn(B, E, n2, k1).astype(f32)
        clo = (rs.randn(B * n2, k1) + 3.0).astype(f32)            # off-centre: a wrong divisor cannot hide
        for use_win in (False, True):
            for use_clo in (False, True):
                for glob in (False, True):
                    out = host(ops.refine_concat(dev(cls), dev(win) if use_win else None, dev(clo) if use_clo else None,
                                                 B, n2, E, glob))
                    # faster_rcnn_meta_arch.py:764-831: [class logits | the E window predictions, proposal-major
                    # (transpose [E, n, k1] -> [n, E, k1]) | closeness]
                    parts = [cls]
                    if use_win:
                        parts.append(win.transpose(0, 2, 1, 3).reshape(B * n2, E * k1))
                    ld = k1 + (E * k1 if use_win else 0) + (k1 if use_clo else 0)
                    assert out.shape == (B * n2, ld)
                    bits(out[:, :ld - (k1 if use_clo else 0)], np.concatenate(parts, 1), "refine_concat copies")
                    if not use_clo:
                        continue
                    got = out[:, ld - k1:]
                    if not glob:
                        bits(got, clo, "refine_concat closeness")
                        continue
                    # :817-821: tf.reduce_mean over every row, padding rows included, tiled; taken per image here
                    # (the reference runs one image per step: frcnn.py predict_with_mtl_results)
                    c3 = clo.astype(np.float64).reshape(B, n2, k1)
                    mean = np.repeat(c3.mean(1), n2, 0)
                    # 4 row-interleaved partial sums of ceil(n2/4) rows, 3 adds, one division
                    depth = -(-n2 // 4) + 3 + 1
                    tol = depth * EPS * np.repeat(np.abs(c3).sum(1), n2, 0) / n2
                    within(got, mean, tol, "global closeness mean B=%d" % B)
                    for b in range(B):
                        assert (got[b * n2:(b + 1) * n2] == got[b * n2]).all(), "one mean per image, tiled"


# ------------------------------------------------------------------------------------------ activation gradients
def _edge_activations(rs, n):
    dn = np.float32(1e-40)                                          # denormal
    y = rs.uniform(-2, 8, n).astype(f32)
    special = np.array([0.0, -0.0, 6.0, np.nextafter(f32(6), f32(7)), np.nextafter(f32(6), f32(0)), dn, -dn,
                        TINY, -TINY, 1e-30, -1e-30, 5.9999995, 6.0000005], f32)
    y[:len(special) * 50] = np.tile(special, 50)
    rs.shuffle(y)
    return y


def test_relu_and_relu6_backward_masks_are_exact(ops):
    rs = np.random.RandomState(4)
    n = 100003
    y = _edge_activations(rs, n)
    dy = rs.randn(n).astype(f32)
    # dx = dy where the forward's output is in the linear range: y > 0 (ReLU), 0 < y < 6 (ReLU6)
    bits(host(ops.relu_bwd(dev(y), dev(dy))), np.where(y > 0, dy, f32(0)), "relu_bwd")
    bits(host(ops.relu6_bwd(dev(y), dev(dy))), np.where((y > 0) & (y < 6), dy, f32(0)), "relu6_bwd")


def _tower_shape():
    cfg = _configs1()
    fr = cfg.model.faster_rcnn
    hw = int(fr.initial_crop_size) // int(fr.maxpool_stride)
    return 2 * int(fr.second_stage_batch_size), hw, hw, 2048       # ResNet-101 block4 output channels


def test_spatial_mean_bwd_fused_and_unfused_against_float64(ops):
    N, H, W, C = _tower_shape()
    assert C % 4 == 0
    rs = np.random.RandomState(6)
    g = torch.Generator(device="cuda").manual_seed(6)
    dy = rs.randn(N, C).astype(f32)
    act = torch.rand((N, H, W, C), generator=g, device="cuda") * 8 - 1
    flat = act.view(-1)
    idx = torch.randint(0, flat.numel(), (4096,), generator=g, device="cuda")
    flat[idx] = dev(np.resize(np.array([0.0, 6.0, 1e-40, -1e-40, np.nextafter(f32(6), f32(0))], f32), 4096))
    # float64 restatement: dx[n, h, w, c] = dy[n, c] / (H * W), kept where 0 < act < 6 (ReLU6) or act > 0 (ReLU).
    # One fp32 division: within 1 ulp of the float64 quotient rounded to fp32; the mask decisions are exact.
    q = dev((dy.astype(np.float64) / (H * W)).astype(f32))
    for m6 in (True, False):
        keep = (act > 0) & (act < 6) if m6 else act > 0
        want = torch.where(keep, q[:, None, None, :].expand(N, H, W, C), torch.zeros((), device="cuda"))
        fused = ops.spatial_mean_bwd(dev(dy), (N, H, W, C), mask_ref=act, mask6=m6)
        assert torch.equal(fused != 0, keep), "fused masked mean backward: mask decisions, relu6=%s" % m6
        ulps = (fused.view(torch.int32).long() - want.view(torch.int32).long()).abs().max().item()
        assert ulps <= 1, "fused masked mean backward: %d ulp from float64, relu6=%s" % (ulps, m6)
        unfused = ops.spatial_mean_bwd(dev(dy), (N, H, W, C))
        unfused = (ops.relu6_bwd if m6 else ops.relu_bwd)(act, unfused, out=unfused)
        assert torch.equal(unfused.view(torch.int32), fused.view(torch.int32)), "fused and unfused paths differ"
        del fused, unfused, want, keep
    # C % 4 != 0: the unfused kernel then the separate mask
    N, H, W, C = 5, 7, 7, 3
    y = _edge_activations(rs, N * H * W * C).reshape(N, H, W, C)
    dy = rs.randn(N, C).astype(f32)
    qn = (dy.astype(np.float64) / (H * W)).astype(f32)[:, None, None, :]
    for m6 in (True, False):
        keep = (y > 0) & (y < 6) if m6 else y > 0
        got = host(ops.spatial_mean_bwd(dev(dy), (N, H, W, C), mask_ref=dev(y), mask6=m6))
        assert ((got != 0) == keep).all(), "unfused masked mean backward C=3: mask decisions, relu6=%s" % m6
        want = np.where(keep, qn, f32(0))
        assert np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32)).max() <= 1, "C=3, relu6=%s" % m6


# --------------------------------------------------------------------------------------------------- optimizer
def test_sgd_momentum_clip_fold_and_bn_refresh_against_float64(ops):
    """The shipped update (ops.sgd_momentum_clip on a ParamStore, ALIGN padding owned by the preceding variable) over two
    steps, with and without the fused shadow-weight fold, then ops.fold_scales and ops.bn_refresh.

    slim.learning.clip_gradient_norms clips each variable by its own norm (tf.clip_by_norm: g * clip / max(|g|, clip))
    after the L2 regulariser's gradient wd * w and the multipliers (trainer.py:389-410); MomentumOptimizer:
    a = m * a + g, w -= lr * a."""
    from mtl_ssl_amd import params
    CH = 1 << 16                                                   # the norm kernel's chunk (NORM_CHUNK)
    clip, lr, mom, gscale = 3.0, 0.05, 0.9, 0.5
    # name: (shape, weight decay, multiplier, fold channels or 0, gradient std)
    spec = {
        "one": ((1,), 0.0, 1.0, 1, 1.0),
        "below_chunk": ((CH - 64,), 4e-5, 1.0, 3, 0.02),       # 65 472 = 3 x 21 824
        "chunk": ((1024, 64), 0.0, 2.0, 64, 0.01),
        "three_chunks_plus": ((3073, 64), 1e-3, 0.5, 0, 0.03),  # 3 x 65 536 + 64
        "frozen": ((10, 100), 1e-3, -1.0, 100, 1.0),
        "wide": ((97, 2048), 0.0, 1.0, 2048, 0.05),             # over 3 chunks, folded per 2048 channels
        "at_clip": ((37,), 0.0, 1.0, 0, 0.0),                   # norm == clip to the last bit
        "above_clip": ((37,), 0.0, 1.0, 0, 0.0),                # norm one ulp above clip
        "ragged": ((5, 3), 2e-4, 1.5, 3, 0.4),
    }
    rs = np.random.RandomState(12)
    ps = params.ParamStore()
    for name, (shape, wd, *_r) in spec.items():
        ps.add(name, shape, "zeros", True, wd)
    values = {n: (rs.randn(*s[0]) * 0.1).astype(f32) for n, s in spec.items()}
    ps.finalize("cuda", values=values)
    names = [sp.name for sp in ps.trainable_specs]
    offs = host(ps.var_offsets).astype(np.int64)
    nv, total = len(names), int(offs[-1])
    wd_v = np.array([spec[n][1] for n in names], f32)
    mult_v = np.array([spec[n][2] for n in names], f32)
    scales = {n: (rs.rand(spec[n][3]) + 0.5).astype(f32) for n in names if spec[n][3]}
    scale_t = {n: dev(s) for n, s in scales.items()}
    for n, s in scale_t.items():
        ps.register_fold(ps.by_name[n], s)
    fold_tab = (ps.eff, ps.fold_ptrs, ps.fold_len)

    def grads_for(step):
        g = np.zeros(total, f32)
        for i, n in enumerate(names):
            sz = int(np.prod(spec[n][0]))
            g[offs[i]:offs[i] + sz] = rs.randn(sz) * spec[n][4]
        # single-element gradients: (g * 0.5) ** 2 = 9 and (next float above 3)^2, so sqrtf gives 3 exactly / one ulp more
        g[offs[names.index("at_clip")] + 5] = 6.0
        g[offs[names.index("above_clip")] + 11] = 2 * np.nextafter(f32(clip), f32(10))
        g[offs[names.index("ragged")]:offs[names.index("ragged")] + 15] *= 40      # clipped hard
        return g

    def reference(w, g, a):
        w, g, a = (x.astype(np.float64) for x in (w, g, a))
        w2, a2, f_all = w.copy(), a.copy(), np.ones(total)
        for i in range(nv):
            s = slice(offs[i], offs[i + 1])                       # the padding belongs to variable i
            if mult_v[i] < 0:
                continue                                           # frozen: not in apply_gradients
            gg = (g[s] * gscale + np.float64(wd_v[i]) * w[s]) * np.float64(mult_v[i])
            nrm = np.sqrt((gg * gg).sum())
            f = clip / max(nrm, clip)
            a2[s] = mom * a[s] + gg * f
            w2[s] = w[s] - lr * a2[s]
            f_all[s] = f
        return w2, a2, f_all

    def check_step(w0, g0, a0, w1, a1, g1, what):
        wr, ar, f = reference(w0, g0, a0)
        gg = np.zeros(total)
        depth = np.zeros(total)
        for i in range(nv):
            s = slice(offs[i], offs[i + 1])
            gg[s] = (g0[s] * gscale + np.float64(wd_v[i]) * w0[s]) * abs(np.float64(mult_v[i]))
            n = offs[i + 1] - offs[i]
            # sum of squares: 4 squares per float4, min(n, 64k)/1024 float4 per lane, 6 wave levels, 2 across the
            # waves, then the chunks in order; all terms >= 0, so the norm is within depth * eps / 2 relative
            depth[s] = 4 * -(-min(n, CH) // 1024) + 6 + 2 + -(-n // CH)
        rel_f = np.where(f < 1, depth * EPS, 0.0)
        # g: 3 roundings; a = m a + g f: 3 more (+ f's error when clipped); w - lr a: 2 more
        tol_a = 4 * EPS * (mom * np.abs(a0) + np.abs(gg) * f) + np.abs(gg) * f * rel_f
        tol_w = 2 * EPS * (np.abs(w0) + lr * np.abs(ar)) + lr * tol_a
        within(a1, ar, tol_a, what + ": accumulator")
        within(w1, wr, tol_w, what + ": weights")
        for i, n in enumerate(names):
            s = slice(offs[i], offs[i + 1])
            if mult_v[i] < 0:
                bits(w1[s], w0[s], what + ": frozen weights")
                bits(a1[s], a0[s], what + ": frozen accumulator")
        assert not g1.any(), what + ": zero_grads leaves zeros (frozen variables included)"

    ps.accum.copy_(dev((rs.randn(total) * 0.01).astype(f32)))
    wdt, mvt = dev(wd_v), dev(mult_v)
    ops.fold_scales(ps)                                             # the shadow weights of the initial values
    for step, fused in ((0, True), (1, True), (2, False)):
        g = grads_for(step)
        ps.grads.copy_(dev(g))
        w0, a0, e0 = host(ps.weights), host(ps.accum), host(ps.eff)
        ops.sgd_momentum_clip(ps.weights, ps.grads, ps.accum, ps.var_offsets, ps.max_var_size, lr, mom, clip,
                              grad_scale=gscale, var_weight_decay=wdt, var_grad_mult=mvt,
                              fold=fold_tab if fused else None, zero_grads=True)
        w1, a1, e1 = host(ps.weights), host(ps.accum), host(ps.eff)
        check_step(w0, g, a0, w1, a1, host(ps.grads), "step %d" % step)
        for i, n in enumerate(names):
            s = slice(offs[i], offs[i + 1])
            if n in scales and fused and mult_v[i] >= 0:
                # eff = w * scale[flat index % K]: one fp32 product of the updated weights, bit-exact
                sc = np.resize(scales[n], offs[i + 1] - offs[i])
                bits(e1[s], (w1[s].astype(np.float64) * sc).astype(f32), "step %d: shadow weights of %s" % (step, n))
            else:
                bits(e1[s], e0[s], "step %d: shadow weights of %s untouched" % (step, n))
    fz = slice(offs[names.index("frozen")], offs[names.index("frozen") + 1])
    bits(host(ps.weights)[fz][:1000], values["frozen"].ravel(), "frozen variable after three steps")
    # ops.fold_scales: every registered fold, frozen variables included
    ps.eff.fill_(float("nan"))
    ops.fold_scales(ps)
    w, e = host(ps.weights), host(ps.eff)
    for i, n in enumerate(names):
        s = slice(offs[i], offs[i + 1])
        if n in scales:
            bits(e[s], (w[s].astype(np.float64) * np.resize(scales[n], offs[i + 1] - offs[i])).astype(f32),
                 "fold_scales " + n)
        else:
            assert np.isnan(e[s]).all(), "fold_scales wrote a variable without a fold: " + n

    # ops.bn_refresh over layers of 3, 256, 300 and 2048 channels, with and without gamma
    chans = [3, 256, 300, 2048]
    guard = 7
    lay = []
    for li, c in enumerate(chans):
        t = {k: dev((rs.randn(c + guard) * 0.5 + (1.0 if k in ("gamma", "inv_std") else 0.0)).astype(f32))
             for k in ("gamma", "beta", "mean", "inv_std", "scale", "shift")}
        t["has_gamma"] = li % 2 == 0
        lay.append(t)
    before = [{k: host(t[k]) for k in ("scale", "shift")} for t in lay]

    def table(k):
        return torch.tensor([t[k].data_ptr() if (k != "gamma" or t["has_gamma"]) else 0 for t in lay],
                            dtype=torch.int64, device="cuda")
    tab = types.SimpleNamespace(n=len(lay), gamma=table("gamma"), beta=table("beta"), mean=table("mean"),
                                inv_std=table("inv_std"), scale=table("scale"), shift=table("shift"),
                                channels=torch.tensor(chans, dtype=torch.int32, device="cuda"), max_c=max(chans))
    ops.bn_refresh(tab)
    for t, c, b0 in zip(lay, chans, before):
        gm, be, mu, iv = (host(t[k]).astype(np.float64)[:c] for k in ("gamma", "beta", "mean", "inv_std"))
        # slim.batch_norm folded: scale = gamma * inv_std (one product: bit-exact), shift = beta - mean * scale
        # (a product and a difference: bound eps * (|beta| + |mean * scale|))
        sc = (gm * iv).astype(f32) if t["has_gamma"] else b0["scale"][:c]
        bits(host(t["scale"])[:c], sc, "bn_refresh scale (%d channels)" % c)
        sh = be - mu * sc.astype(np.float64)
        within(host(t["shift"])[:c], sh, EPS * (np.abs(be) + np.abs(mu * sc)), "bn_refresh shift (%d channels)" % c)
        bits(host(t["scale"])[c:], b0["scale"][c:], "bn_refresh: scale past the layer's channels")
        bits(host(t["shift"])[c:], b0["shift"][c:], "bn_refresh: shift past the layer's channels")
