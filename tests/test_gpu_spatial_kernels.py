"""GPU: the spatial kernels between trunk and heads (RoI crop + pool, position-sensitive RoI, bilinear resize, max /
average pooling, depthwise 3x3, bn_param_grads, the spatial mean, channel copies, box clipping, window expansion), each
against a float64 NumPy restatement (tests/spatial_ref.py) with ELEMENTWISE bounds that follow from the arithmetic
(eps = 2^-23; one fp32 rounding is at most eps/2 relative):
  * data movement and comparisons are bit-exact;
  * a fixed sequence of r roundings is within r * eps/2 of float64, relative to the operands named at the test;
  * a sum is within depth * eps * sum|terms| of float64, `depth` being the kernel's own longest chain of additions
    (eps per step instead of eps/2 covers the second-order terms and a rounding of each term).
Indices (sampling taps, validity, arg-max routing) are never given a tolerance: the references restate the float32
coordinate arithmetic step by step (ops.hip is built with -ffp-contract=off), so a tap that differs is a failure.
No code path of the models emits a depthwise dilation other than 1 (nn.DepthwiseBN is always built with dilation 1 by
mobilenet.py), so the depthwise cases use dilation 1 only."""
import os

import numpy as np
import pytest
import torch

from tests import spatial_ref as S
from tests.f64_check import EPS, bits, dev, host, within

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U = EPS / 2                                                        # one rounding


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


# ------------------------------------------------------------------------------------------------ RoI crop + pool
# (B,H,W,C, RoIs, crop, pool k, pool stride): ResNet-101 / MobileNet / Inception-ResNet-v2 second-stage inputs
ROI_SITES = {"resnet101": (2, 38, 64, 1024, 512, 14, 2, 2), "mobilenet": (2, 38, 50, 512, 512, 7, 1, 1),
             "inception_resnet_v2": (2, 50, 84, 1088, 512, 17, 1, 1)}


def stripes(C):
    """Channels checked at the full-size sites. The channel-sliced forward kernel deals eight C/8 slices to the XCDs; the
    stripes are the FIRST float4 of the even slices and the LAST float4 of the odd ones, 32 channels in all (C = 1024:
    0-3, 252-255, 256-259, 508-511, 512-515, 764-767, 768-771, 1020-1023). They were thinned from both ends of every
    slice (64 channels) to keep the file's wall time near that of its two sibling files together; every slice, a slice
    start and a slice end, and the map's first and last float4 remain."""
    s = C // 8
    return np.concatenate([np.r_[k * s:k * s + 4] if k % 2 == 0 else np.r_[(k + 1) * s - 4:(k + 1) * s] for k in range(8)])


def _exact_fraction(n, rs, count):
    """k / (n-1) values whose float32 product with (n-1) is exactly the integer k: samples land ON a map row."""
    k = np.arange(1, n - 1)
    v = (k / (n - 1)).astype(f32)
    ok = (v * f32(n - 1)) == k.astype(f32)
    assert ok.sum() >= count
    return v[ok][rs.permutation(int(ok.sum()))[:count]]


def roi_boxes(R, H, W, rs, B=2):
    """Random boxes (some poking outside) plus the legal edge cases: the full image, zero area, flipped, wholly outside
    on each side, straddling each border, sub-pixel, samples exactly on integer rows / columns and exactly on H-1 / W-1,
    one float32 step outside; box_ind in arbitrary order."""
    yx = rs.rand(R, 2) * 0.9 - 0.05
    hw = rs.rand(R, 2) * 0.6 + 0.02
    b = np.concatenate([yx, yx + hw], 1).astype(f32)
    up, dn = np.nextafter(f32(1), f32(2)), np.nextafter(f32(0), f32(-1))
    ey, ex = _exact_fraction(H, rs, 4), _exact_fraction(W, rs, 4)
    edge = [[0, 0, 1, 1], [0.3, 0.3, 0.3, 0.3], [1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 0], [0.8, 0.7, 0.2, 0.1],
            [0.2, 0.7, 0.8, 0.1], [-0.5, 0.2, -0.1, 0.6], [1.1, 0.2, 1.5, 0.6], [0.2, -0.5, 0.6, -0.1], [0.2, 1.1, 0.6, 1.5],
            [-0.2, 0.3, 0.3, 0.7], [0.7, 0.3, 1.2, 0.7], [0.3, -0.2, 0.7, 0.3], [0.3, 0.7, 0.7, 1.2], [-0.3, -0.3, 1.3, 1.3],
            [0.4, 0.4, 0.401, 0.401], [0.4, 0.4, 0.4 + 0.3 / H, 0.4 + 0.3 / W], [up, up, up, up], [dn, dn, dn, dn],
            [0, 0, up, up], [dn, dn, 1, 1], [ey[0], ex[0], ey[0], ex[0]], [ey[1], ex[1], ey[1], ex[1]],
            [ey[2], ex[2], 1, 1], [1, 1, ey[3], ex[3]], [0, 0, ey[3], ex[3]]]
    b[:len(edge)] = np.array(edge, f32)
    return b, rs.randint(0, B, R).astype(np.int32)


def _roi_fwd(ops, feat, boxes, bi, crop, pk, ps, kernel, monkeypatch):
    if kernel == "xcd":
        monkeypatch.setenv("MTLSSL_ROI_FWD", "xcd")
    else:
        monkeypatch.delenv("MTLSSL_ROI_FWD", raising=False)
    return ops.roi_crop_pool_fwd(feat, boxes, bi, crop, pk, ps)


def check_roi_fwd(out, am, feat_s, boxes, bi, crop, pk, ps, idx, what):
    """-> the verified arg-max positions [R,PH,PW,len(idx)] (zeros when pk == 1)."""
    val, amax, valid = S.crop_and_resize(feat_s, boxes, bi, crop)
    win, wa = S.pool_windows(val, pk, ps), S.pool_windows(amax, pk, ps)
    wv = S.pool_windows(np.broadcast_to(valid[..., None], val.shape), pk, ps)
    # a sample is three lerps a + (b - a) * l of three roundings each (sub, mul, add). With A = max |corner| and l < 1:
    # |b - a| <= 2A, so one lerp is off by at most (2 * 2A * l + A) * eps/2 <= 5A eps/2; the third lerp carries the first
    # two through ((1 - yl) * 5 + yl * 5 = 5) and adds its own 5: 10 roundings of A = 5 * eps * A
    tol = 5 * EPS * wa
    got = host(out)[..., idx]
    assert (got[(~wv).all(3)] == 0).all(), what + ": a window of extrapolated samples must be exactly 0"
    if pk == 1:
        assert am is None
        within(got, win[:, :, :, 0], tol[:, :, :, 0], what + ": crop")
        assert (got[~wv[:, :, :, 0]] == 0).all(), what + ": an extrapolated sample must be exactly 0"
        assert (wv[:, :, :, 0] & (val == 0)).sum() < wv.sum()                     # (valid samples exist)
        return np.zeros(got.shape, np.int64)
    sel = host(am)[..., idx].astype(np.int64)
    assert sel.max() < pk * pk, what + ": arg-max byte outside the window"
    pick = lambda a, i: np.take_along_axis(a, i[:, :, :, None, :], 3)[:, :, :, 0]
    top = win.argmax(3)
    v_sel, t_sel = pick(win, sel), pick(tol, sel)
    # the kernel chose `sel` because its fp32 value was >= the fp32 value of the float64 winner: in float64 the chosen
    # sample may trail the maximum by the two samples' own bounds, no more — no element is excluded
    within(v_sel, win.max(3), t_sel + pick(tol, top), what + ": sample named by the arg-max byte vs the window maximum")
    within(got, v_sel, t_sel, what + ": pooled value vs the sample its arg-max byte names")
    # exact ties: extrapolated samples are exactly 0; where every valid sample of the window is negative beyond its
    # bound the maximum is that 0 and the FIRST extrapolated position in window order is recorded
    lost = (~wv) | (win < -tol)
    tie = lost.all(3) & (~wv).any(3)
    assert tie.sum() > 100 and ((~wv).sum(3)[tie] > 1).any(), "the box set must produce tied windows"
    first = np.argmax(~wv, 3)
    bad = tie & (sel != first)
    assert not bad.any(), "%s: %d tied windows do not record the first maximum, e.g. %s" % (what, bad.sum(), np.argwhere(bad)[0])
    assert (got[tie] == 0).all()
    return sel


@pytest.mark.parametrize("kernel", ["cell", "xcd"])
@pytest.mark.parametrize("site", list(ROI_SITES))
def test_roi_crop_pool_forward_against_float64(ops, site, kernel, monkeypatch):
    B, H, W, C, R, crop, pk, ps = ROI_SITES[site]
    rs = np.random.RandomState(H * W)
    feat = rs.randn(B, H, W, C).astype(f32)
    boxes, bi = roi_boxes(R, H, W, rs)
    idx = stripes(C)
    # the edge cases are really there: samples exactly on the last row / column, on interior integers, just outside
    pos, valid, _, _, frac = S.crop_axis(boxes[:, 0], boxes[:, 2], H, crop)
    assert (pos[valid] == H - 1).any() and ((frac == 0) & valid & (pos > 0) & (pos < H - 1)).any() and (~valid).any()
    out, am = _roi_fwd(ops, dev(feat), dev(boxes), dev(bi), crop, pk, ps, kernel, monkeypatch)
    check_roi_fwd(out, am, feat[..., idx], boxes, bi, crop, pk, ps, idx, "%s %s" % (site, kernel))


@pytest.mark.parametrize("kernel", ["cell", "xcd"])
@pytest.mark.parametrize("crop,pk,ps", [(1, 1, 1), (7, 2, 1), (9, 2, 3), (8, 3, 2)])
def test_roi_crop_pool_forward_small_geometries(ops, crop, pk, ps, kernel, monkeypatch):
    """crop == 1 (the centre form) and pool_stride != pool_k, every channel checked. (pk = 3 always runs the
    block-per-cell kernel: the channel-sliced one takes pk <= 2.)"""
    rs = np.random.RandomState(crop)
    feat = rs.randn(2, 13, 17, 64).astype(f32)
    boxes, bi = roi_boxes(96, 13, 17, rs)
    out, am = _roi_fwd(ops, dev(feat), dev(boxes), dev(bi), crop, pk, ps, kernel, monkeypatch)
    # the same checks as at the call sites, the extrapolated-sample and first-index tie rules included
    check_roi_fwd(out, am, feat, boxes, bi, crop, pk, ps, np.arange(64), "crop %d pool %d/%d %s" % (crop, pk, ps, kernel))


def _fixed_point_exponent(dout):
    """e of k_roi_crop_pool_bwd_lds: M = max |dout| in [2^(e-1), 2^e), from M's exponent bits, at least -90."""
    mbits = int(np.abs(dout).max().astype(f32).view(np.uint32))
    return max((mbits >> 23) - 126, -90)


def check_roi_bwd(ops, dout, sel, am, feat_shape, boxes, bi, crop, pk, ps, idx, what, algos=(1, 2), base_seed=5):
    """Both algorithms, overwrite and accumulate, against the float64 scatter on the channels `idx`."""
    grad, n, sabs = S.roi_crop_pool_bwd(dout[..., idx], sel, feat_shape[:3] + (len(idx),), boxes, bi, crop, pk, ps)
    base = np.random.RandomState(base_seed).randn(*feat_shape).astype(f32)
    bs = base[..., idx].astype(np.float64)
    e = _fixed_point_exponent(dout)
    # every contribution g * (1-yl) * (1-xl) is formed in fp32 by four roundings (1-yl, * g, 1-xl, *): 4 * eps/2 of |c|
    prod = 2 * EPS * sabs
    for algo in algos:
        for acc in (0, 1):
            d = ops.roi_crop_pool_bwd(dev(dout), am, feat_shape, dev(boxes), dev(bi), crop, pk, ps,
                                      dfeat=dev(base) if acc else torch.full(feat_shape, float("nan"), device="cuda"),
                                      accumulate=bool(acc), algo=algo)
            got = host(d)[..., idx]
            ref = grad + bs * acc
            if algo == 2:
                # float atomics onto the (zeroed or prior) cell in arrival order: a chain of n (+1) additions
                tol = prod + (n + acc) * EPS * (sabs + np.abs(bs) * acc)
            else:
                # 64-bit fixed point with step 2^(e-30), e as the kernel takes it from M = max |dout| in [2^(e-1), 2^e):
                # one rint per addend is off by at most half a step, 2^(e-31), and the integer sum is exact; then one
                # rounding on write-out and one more when accumulating. (n * M * 2^-31 would be up to twice too tight:
                # the step follows 2^e, not M.)
                tol = prod + n * 2.0 ** (e - 31) + EPS * np.abs(grad) + acc * EPS * np.abs(ref)
            within(got, ref, tol, "%s algo %d accumulate %d" % (what, algo, acc))
            bits(got[n == 0], (base[..., idx] if acc else np.zeros_like(got))[n == 0],
                 "%s algo %d accumulate %d: cells no RoI touches" % (what, algo, acc))
    return grad, n, sabs


@pytest.mark.parametrize("site", list(ROI_SITES))
def test_roi_crop_pool_backward_against_float64(ops, site, monkeypatch):
    B, H, W, C, R, crop, pk, ps = ROI_SITES[site]
    rs = np.random.RandomState(H + W)
    feat = rs.randn(B, H, W, C).astype(f32)
    boxes, bi = roi_boxes(R, H, W, rs)
    idx = stripes(C)
    out, am = _roi_fwd(ops, dev(feat), dev(boxes), dev(bi), crop, pk, ps, "cell", monkeypatch)
    sel = check_roi_fwd(out, am, feat[..., idx], boxes, bi, crop, pk, ps, idx, site)      # the bytes the scatter follows
    dout = rs.randn(*out.shape).astype(f32)
    _, n, _ = check_roi_bwd(ops, dout, sel if pk > 1 else None, am, (B, H, W, C), boxes, bi, crop, pk, ps, idx, site)
    assert n.max() > 50                  # (cells no RoI touches: the piled case below leaves a whole image untouched)


def test_roi_crop_pool_backward_piled_rois_and_long_lists(ops, monkeypatch):
    """More RoIs per image than one pass of the LDS lists holds, RoIs piled onto one box and onto sub-pixel boxes (many
    lanes of one instruction hit one cell), an image without any RoI; every channel checked."""
    B, H, W, C, R, crop = 3, 19, 25, 48, 2300, 7
    rs = np.random.RandomState(9)
    boxes, bi = roi_boxes(R, H, W, rs)
    boxes[100:R // 4, 2:] = boxes[100:R // 4, :2] + (0.004 * rs.rand(R // 4 - 100, 2)).astype(f32)
    boxes[R // 4:R // 2] = boxes[50]
    bi = (rs.randint(0, 2, R) * 2).astype(np.int32)                              # images 0 and 2 only
    dout = rs.randn(R, crop, crop, C).astype(f32)
    grad, n, _ = check_roi_bwd(ops, dout, None, None, (B, H, W, C), boxes, bi, crop, 1, 1, np.arange(C), "piled")
    assert n.max() > 1000 and (n[1] == 0).all()


def test_roi_crop_pool_backward_wide_dynamic_range(ops, monkeypatch):
    """One gradient of magnitude ~1 among gradients of ~2^-20: the fixed-point step is set by the large one
    (M * 2^-30), most small contributions fall near or below it, and the SAME absolute bound n * 2^(e-31) must hold."""
    B, H, W, C, R, crop, pk, ps = ROI_SITES["mobilenet"]
    rs = np.random.RandomState(21)
    boxes, bi = roi_boxes(R, H, W, rs)
    dout = (rs.randn(R, crop, crop, C) * 2.0 ** -20).astype(f32)
    dout[40, 3, 3, 0] = 1.5
    assert _fixed_point_exponent(dout) == 1
    idx = stripes(C)
    grad, n, sabs = check_roi_bwd(ops, dout, None, None, (B, H, W, C), boxes, bi, crop, pk, ps, idx, "wide range", algos=(1,))
    assert np.median(sabs[n > 0] / n[n > 0]) < 2.0 ** -21                          # (the small ones do dominate the map)


def test_roi_crop_pool_backward_non_finite_gradient(ops):
    """include/mtlssl_hip.h: 'A non-finite value in dout turns the whole map into NaN (LDS kernel)'."""
    rs = np.random.RandomState(2)
    boxes, bi = roi_boxes(64, 13, 17, rs)
    dout = rs.randn(64, 7, 7, 32).astype(f32)
    dout[5, 1, 2, 3] = np.inf
    for acc in (False, True):
        d = ops.roi_crop_pool_bwd(dev(dout), None, (2, 13, 17, 32), dev(boxes), dev(bi), 7, 1, 1,
                                  dfeat=torch.zeros(2, 13, 17, 32, device="cuda"), accumulate=acc, algo=1)
        assert np.isnan(host(d)).all()


# --------------------------------------------------------------------------------------- position-sensitive RoI
def _rfcn_channels():
    """Score-map depths rfcn.RfcnBoxPredictor builds for the R-FCN VOC config: nb * (num_classes + 1) class scores and
    nb * num_classes * 4 box encodings, nb = 3 x 3 bins, crop 18 x 18."""
    from mtl_ssl_amd import config
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "rfcn_resnet101_voc_mtl.config")).read())
    fr = cfg.model.faster_rcnn
    p = fr.second_stage_box_predictor.rfcn_box_predictor
    bins = (int(p.num_spatial_bins_height), int(p.num_spatial_bins_width))
    k = int(fr.num_classes)
    return bins, (int(p.crop_height), int(p.crop_width)), (bins[0] * bins[1] * (k + 1), bins[0] * bins[1] * k * 4)


@pytest.mark.parametrize("which", [0, 1])
def test_psroi_forward_and_backward_against_float64(ops, which):
    bins, crop, depths = _rfcn_channels()
    assert bins == (3, 3) and crop == (18, 18) and depths == (9 * 21, 9 * 20 * 4)
    Ct = depths[which]
    B, H, W, R = 2, 38, 64, 600
    rs = np.random.RandomState(Ct)
    fmap = rs.randn(B, H, W, Ct).astype(f32)
    boxes, bi = roi_boxes(R, H, W, rs)
    bi = np.sort(bi)[rs.permutation(R)].astype(np.int32)
    val, sumA = S.psroi(fmap, boxes, bi, crop, bins)
    got = ops.psroi_fwd(dev(fmap), dev(boxes), dev(bi), crop, bins)
    # a sample is within 5 eps of its max |corner| (three lerps, see the RoI forward); a channel's 9 * 36 samples are
    # summed in chains of 36 (a bin) + 9 (the bins); then * (1 / 324): the rounded reciprocal and the product
    nb, ns = bins[0] * bins[1], (crop[0] // bins[0]) * (crop[1] // bins[1])
    within(host(got), val, (5 + ns + nb) * EPS * sumA + EPS * np.abs(val), "psroi forward")
    dout = rs.randn(R, Ct // nb).astype(f32)
    grad, n, sabs = S.psroi_bwd(dout, fmap.shape, boxes, bi, crop, bins)
    base = rs.randn(*fmap.shape).astype(f32)
    # a term dout * inv * (wy * wx): wy and wx are fp32 sums of at most 2 * 6 rounded weights (13 roundings each), the
    # reciprocal and three products: 30 roundings = 15 eps of |term|; n terms are added in RoI order, then `+=` once
    for acc in (0, 1):
        d = ops.psroi_bwd(dev(dout), fmap.shape, dev(boxes), dev(bi), crop, bins, dfmap=dev(base) if acc else None)
        ref = grad + acc * base.astype(np.float64)
        within(host(d), ref, (15 + n) * EPS * sabs + EPS * np.abs(ref), "psroi backward, accumulate %d" % acc)
        bits(host(d)[n == 0], (base if acc else np.zeros_like(base))[n == 0], "psroi backward: untouched cells")


# ------------------------------------------------------------------------------------------------ bilinear resize
RESIZE_SHAPES = [(38, 64), (64, 38), (38, 50), (50, 38), (50, 84), (84, 50), (64, 64), (1, 1), (1, 7), (7, 1), (128, 128)]
# every scale n / 64 is exact in fp32; 37 and 23 outputs give scales that round (50/37, 84/37, 38/23, 64/23), so that the
# backward gather's candidate range (floor((iy-1)/s) - 1 .. ceil((iy+1)/s) + 1) works on inexact quotients as well
RESIZE_CASES = [(h, w, 2, 64, 64) for h, w in RESIZE_SHAPES] + [(50, 84, 8, 64, 64), (50, 84, 2, 37, 37), (38, 64, 2, 23, 23),
                                                                 (7, 5, 2, 37, 23)]


@pytest.mark.parametrize("H,W,C,OH,OW", RESIZE_CASES)
def test_resize_bilinear_against_float64(ops, H, W, C, OH, OW):
    rs = np.random.RandomState(H * 131 + W + OH)
    x = rs.randn(2, H, W, C).astype(f32)
    val, amax = S.resize_bilinear(x, OH, OW)
    y = host(ops.resize_bilinear_fwd(dev(x), OH, OW))
    tol_f = 5 * EPS * amax                                     # three lerps of three roundings, as in the RoI forward
    within(y, val, tol_f, "resize forward")
    if (H, W) == (OH, OW):
        bits(y, x, "resize to the same size is the identity")
    g = rs.randn(2, OH, OW, C).astype(f32)
    grad, n, sabs = S.resize_bilinear_bwd(g, x.shape)
    dx = host(ops.resize_bilinear_bwd(dev(g), x.shape))
    # a term g * (1-yl) * (1-xl): four roundings (two complements, two products) = 2 eps of |term|; the gather adds its n
    # terms in a fixed order (n * eps * sum|terms|), then `dx += acc` rounds once more
    tol_b = (2 + n) * EPS * sabs + EPS * np.abs(grad)
    within(dx, grad, tol_b, "resize backward into zeros")
    assert (dx[n == 0] == 0).all()
    # <resize(x), g> = <x, resize_bwd(g)>: catches a forward / backward disagreement about a boundary tap
    lhs, rhs = (y.astype(np.float64) * g).sum(), (x.astype(np.float64) * dx).sum()
    assert abs(lhs - rhs) <= (tol_f * np.abs(g)).sum() + (tol_b * np.abs(x)).sum(), (lhs, rhs)


def test_resize_bilinear_backward_accumulates_into_a_filled_buffer(ops):
    """The C entry point adds into dx (the Python wrapper hands it zeros): call it on a pre-filled buffer."""
    from mtl_ssl_amd.lib import lib, ptr
    rs = np.random.RandomState(4)
    H, W, C = 50, 84, 2
    g = rs.randn(2, 64, 64, C).astype(f32)
    base = rs.randn(2, H, W, C).astype(f32)
    grad, n, sabs = S.resize_bilinear_bwd(g, base.shape)
    dx = dev(base)
    lib().resize_bilinear_bwd(ptr(dev(g)), ptr(dx), 2, H, W, C, 64, 64, ops._stream())
    ref = grad + base.astype(np.float64)
    within(host(dx), ref, (2 + n) * EPS * sabs + EPS * np.abs(ref), "resize backward into a filled buffer")
    bits(host(dx)[n == 0], base[n == 0], "cells no output pixel reads")


# ------------------------------------------------------------------------------------------------------- pooling
# ResNet stem; Inception-ResNet-v2 at 800 x 1333: both stem pools (after Conv2d_2b and Conv2d_4a) and Mixed_6a's pool
# into the 1088-wide map — inception_resnet_v2.py builds these three with SAME padding — and Mixed_7a's VALID pool of the
# 17 x 17 crops into the 2080-wide map. Mixed_7a runs on 64 crops instead of a step's RoI count: every crop is pooled
# alone, and the float64 reference of 64 of them is already 0.5 GB.
MAXPOOL_SITES = [((2, 300, 512, 64), "SAME", None), ((2, 400, 667, 64), "SAME", None), ((2, 200, 334, 192), "SAME", None),
                 ((2, 100, 167, 320), "SAME", (1088, 768)), ((64, 17, 17, 1088), "VALID", (2080, 992))]


@pytest.mark.parametrize("shape,padding,into", MAXPOOL_SITES)
def test_maxpool_3x3_stride_2_at_call_sites(ops, shape, padding, into):
    rs = np.random.RandomState(shape[1])
    rng = np.random.default_rng(shape[1])                                      # float32 draws for the large maps
    for ties in (False, True):
        # ties: small integers, so that most windows hold several equal maxima and the first-in-window-order rule decides
        x = rng.integers(0, 3, shape).astype(f32) if ties else rng.standard_normal(shape, dtype=f32)
        yref = S.max_pool(x, 3, 2, padding)
        xd = dev(x)
        if into is None:
            y, pads = ops.maxpool_fwd(xd, 3, 2, padding)
            gy = dev(rs.randn(*yref.shape).astype(f32))
        else:                                            # the pooling branch writes its channel slice of the concat map
            wide, c0 = into
            big = torch.full(yref.shape[:3] + (wide,), float("nan"), device="cuda")
            y, pads = ops.maxpool_fwd(xd, 3, 2, padding, out=big[..., c0:c0 + shape[3]])
            assert torch.isnan(big[..., :c0]).all() and torch.isnan(big[..., c0 + shape[3]:]).all()
            gbig = dev(rs.randn(*big.shape).astype(f32))
            gy = gbig[..., c0:c0 + shape[3]]
        bits(host(y), yref, "max-pool forward")
        grad, n, sabs = S.max_pool_bwd(x, host(gy), 3, 2, padding)
        dx = host(ops.maxpool_bwd(xd, y, gy, 3, 2, pads))
        # an element is the first maximum of at most four 3x3/2 windows: a chain of n <= 4 additions of exact terms
        assert n.max() <= 4 and (not ties or n.max() == 4)
        within(dx, grad, n * EPS * sabs, "max-pool backward")
        assert (dx[n == 0] == 0).all()


@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("k,stride", [(2, 1), (2, 2), (3, 1), (3, 2), (5, 1), (5, 2)])
@pytest.mark.parametrize("shape", [(2, 100, 167, 192), (2, 9, 12, 8), (1, 10, 7, 8)])
def test_avgpool_against_float64(ops, shape, k, stride, padding):
    """(2,100,167,192) is Mixed_5b's branch-3 input at 800 x 1333; odd and even small maps."""
    rs = np.random.RandomState(k * 7 + stride)
    x = rs.randn(*shape).astype(f32)
    val, cnt, sabs = S.avg_pool(x, k, stride, padding)
    y, pads = ops.avgpool_fwd(dev(x), k, stride, padding)
    assert tuple(y.shape) == val.shape
    # at most k*k terms added in a chain, then one division by the in-bounds count
    tol = (k * k * EPS * sabs) / cnt[None, :, :, None] + EPS * np.abs(val)
    got = host(y)
    OH, OW = cnt.shape
    edge = np.zeros((OH, OW), bool)
    edge[[0, -1], :] = True
    edge[:, [0, -1]] = True
    corner = np.zeros((OH, OW), bool)
    corner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    for name, m in (("corner", corner), ("edge", edge & ~corner), ("interior", ~edge)):
        if m.any():
            within(got[:, m], val[:, m], tol[:, m], "avg-pool forward, %s windows" % name)
    assert cnt.max() <= k * k and (padding == "VALID") == (cnt.min() == k * k)     # (SAME has partial windows)
    ones, _ = ops.avgpool_fwd(torch.ones(shape, device="cuda"), k, stride, padding)
    assert (host(ones) == 1).all(), "a window of ones averages to exactly 1 whatever its in-bounds count"
    gy = rs.randn(*val.shape).astype(f32)
    grad, n, sg = S.avg_pool_bwd(gy, shape, k, stride, padding)
    dx = host(ops.avgpool_bwd(dev(gy), shape, k, stride, pads))
    # each term dy / count is rounded once, at most k*k of them are added in a chain
    within(dx, grad, (1 + n) * EPS * sg, "avg-pool backward")
    assert (dx[n == 0] == 0).all()
    for name, m in (("top row", np.s_[:, 0]), ("left column", np.s_[:, :, 0]), ("bottom row", np.s_[:, -1]), ("right column", np.s_[:, :, -1])):
        within(dx[m], grad[m], ((1 + n) * EPS * sg)[m], "avg-pool backward, " + name)


# ----------------------------------------------------------------------------------------------------- depthwise
def mobilenet_depthwise_layers():
    """(N,H,W,C,stride) of every depthwise layer mobilenet.py builds for the MobileNet VOC config on a 600 x 800 image
    (the 38 x 50 map), batch 2, walked through mobilenet._CONV_DEFS, plus the RoI stage on 2 x 256 crops of 7 x 7."""
    from mtl_ssl_amd import mobilenet
    H, W, cin, out = 600, 800, 3, []
    for kind, stride, depth in mobilenet._CONV_DEFS:
        if kind == "sep":
            out.append((2, H, W, cin, stride))
        H, W, cin = -(-H // stride), -(-W // stride), depth
    assert (H, W, cin) == (38, 50, 512)
    out += [(512, 7, 7, 512, 2), (512, 4, 4, 1024, 1)]                          # Conv2d_12 / Conv2d_13 depthwise stages
    return out


DW_LAYERS = [(2, 300, 400, 32, 1), (2, 300, 400, 64, 2), (2, 150, 200, 128, 1), (2, 150, 200, 128, 2), (2, 75, 100, 256, 1),
             (2, 75, 100, 256, 2), (2, 38, 50, 512, 1), (512, 7, 7, 512, 2), (512, 4, 4, 1024, 1)]
# reduce_plan branches: C/4 = 9 (dead quads inside a block of 16), P < 2*PL, P odd, P = one more than a multiple of
# per_chunk (C = 36: PL = 16; P = 2*16*16+1 = 513 -> chunks 17, per_chunk 32, the last chunk holds one pixel)
DW_EXTRA = [(1, 19, 27, 36, 1), (1, 3, 5, 36, 1), (1, 5, 5, 512, 1), (1, 19, 27, 36, 2), (1, 1, 1, 8, 1)]


def reduce_plan(P, C):
    """depthwise.hip reduce_plan restated -> (CQ, PL, chunks, per_chunk, depth): the longest chain of additions a term
    passes through = a lane's terms of one chunk + the PL-1 block-reduction adds + a fold lane's chunks + 6 butterfly
    levels."""
    CQ = 64
    while CQ > 1 and CQ // 2 >= C // 4:
        CQ //= 2
    PL = 256 // CQ
    bx = -(-(C // 4) // CQ)
    chunks = max(1, min(2048 // bx, -(-P // (2 * PL)), 2048))
    per_chunk = -(-(-(-max(P, 1) // chunks)) // PL) * PL
    chunks = -(-max(P, 1) // per_chunk)
    return CQ, PL, chunks, per_chunk, per_chunk // PL + (PL - 1) + -(-chunks // 64) + 6


@pytest.mark.parametrize("N,H,W,C,stride", DW_LAYERS + DW_EXTRA)
def test_depthwise_against_float64(ops, N, H, W, C, stride):
    rs = np.random.RandomState(H * C + stride)
    x = rs.randn(N, H, W, C).astype(f32)
    w = (rs.randn(3, 3, C) * 0.3).astype(f32)
    bias = rs.randn(C).astype(f32)
    d = ops.conv_desc(x.shape, (3, 3, C, C), stride, 1, "SAME")
    val, sabs = S.depthwise(x, w, stride, 1, bias)
    # nine multiply-adds in a chain (fused or not: at most one rounding per product and per addition) and the bias
    tol = (9 + 1) * EPS * sabs
    within(host(ops.depthwise_fwd(d, dev(x), dev(w), dev(bias), ops.EPI_BIAS)), val, tol, "depthwise forward + bias")
    v0, s0 = S.depthwise(x, w, stride, 1)
    within(host(ops.depthwise_fwd(d, dev(x), dev(w))), v0, 9 * EPS * s0, "depthwise forward")
    for epi, hi in ((ops.EPI_RELU, np.inf), (ops.EPI_RELU6, 6.0)):
        y = host(ops.depthwise_fwd(d, dev(x), dev(w), dev(bias), ops.EPI_BIAS | epi))
        within(y, np.clip(val, 0, hi), tol, "depthwise forward + activation")
        assert (y[val < -tol] == 0).all() and (y >= 0).all() and (y <= hi).all() and (y[val > hi + tol] == hi).all()
    g = rs.randn(*val.shape).astype(f32)
    dx, sx = S.depthwise_dgrad(g, w, x.shape, stride, 1)
    within(host(ops.depthwise_dgrad(d, dev(g), dev(w))), dx, 9 * EPS * sx, "depthwise dgrad")
    # masks: the activation that produced x placed EXACTLY at 0 and at 6 (the gradient of ReLU / ReLU6 is 0 there)
    m = (rs.randn(*x.shape) * 4).astype(f32)
    m.reshape(-1)[::7] = 0.0
    m.reshape(-1)[3::7] = 6.0
    m.reshape(-1)[5::7] = np.nextafter(f32(6), f32(0))
    for epi, on in ((ops.EPI_MASK, m > 0), (ops.EPI_MASK6, (m > 0) & (m < 6))):
        got = host(ops.depthwise_dgrad(d, dev(g), dev(w), mask_ref=dev(m), epilogue=epi))
        within(got, np.where(on, dx, 0.0), 9 * EPS * sx, "depthwise dgrad + mask")
        assert (got[~on] == 0).all(), "the gradient must be exactly 0 where the activation is at 0 or 6"
    dw, sw = S.depthwise_wgrad(x, g, stride, 1)
    depth = reduce_plan(g.size // C, C)[4]
    scale = (rs.rand(C) + 0.5).astype(f32)
    prior = rs.randn(3, 3, C).astype(f32)
    for sc in (None, scale):
        for beta in (0.0, 1.0):
            got = host(ops.depthwise_wgrad(d, dev(x), dev(g), dev(prior), out_scale=None if sc is None else dev(sc), beta=beta))
            s = 1.0 if sc is None else sc.astype(np.float64)
            ref = s * dw + beta * prior
            # the reduction bound with the kernel's depth (a product rounds once more), one rounding for out_scale, one
            # for beta * dw + s
            within(got, ref, (depth + 2) * EPS * s * sw + EPS * np.abs(ref), "depthwise wgrad, scale %s beta %g" % (sc is not None, beta))


def test_depthwise_activations_exactly_at_0_and_6(ops):
    """Integer inputs, filters and biases: every sum is exact in fp32, so the pre-activation lands EXACTLY on 0 and on 6
    in many places and the output must equal the clipped exact value bit for bit."""
    rs = np.random.RandomState(0)
    x = rs.randint(-2, 3, (2, 9, 11, 16)).astype(f32)
    w = rs.randint(-1, 2, (3, 3, 16)).astype(f32)
    bias = rs.randint(0, 7, 16).astype(f32)
    d = ops.conv_desc(x.shape, (3, 3, 16, 16), 1, 1, "SAME")
    val, _ = S.depthwise(x, w, 1, 1, bias)
    assert (val == 0).sum() > 20 and (val == 6).sum() > 20
    bits(host(ops.depthwise_fwd(d, dev(x), dev(w), dev(bias), ops.EPI_BIAS | ops.EPI_RELU)), np.maximum(val, 0), "relu")
    bits(host(ops.depthwise_fwd(d, dev(x), dev(w), dev(bias), ops.EPI_BIAS | ops.EPI_RELU6)), np.clip(val, 0, 6), "relu6")


# ---------------------------------------------------------------------------------------------- bn_param_grads
@pytest.mark.parametrize("C", [32, 36, 64, 1024])
@pytest.mark.parametrize("rows", [0, 1, 7, 2 * 19 * 27, 300000])
def test_bn_param_grads_against_float64(ops, rows, C):
    rs = np.random.RandomState(rows % 1000 + C)
    rng = np.random.default_rng(rows % 1000 + C)                              # float32 draws: 300000 x 1024 stays at 1.2 GB
    gamma = (rs.rand(C) + 0.5).astype(f32) * np.where(rs.rand(C) < 0.5, -1, 1).astype(f32)
    gamma[1::8] = 0.001                                  # tiny gamma: y - beta is 1000 x smaller than y's spread elsewhere
    gamma[2::16] = 0.0
    beta = rs.randn(C).astype(f32)
    y = rng.standard_normal((rows, C), dtype=f32)
    y *= gamma
    y += beta
    g = rng.standard_normal((rows, C), dtype=f32)
    blocks = [S.bn_param_grads(y[a:a + 32768], g[a:a + 32768], gamma, beta) for a in range(0, max(rows, 1), 32768)]
    dgamma, dbeta, s_gy, s_g = (sum(b[k] for b in blocks) for k in range(4))          # float64 by row blocks
    depth = reduce_plan(rows, C)[4]
    prior = rs.randn(2, C).astype(f32)
    nz = gamma != 0
    ag = np.abs(np.where(nz, gamma, 1.0).astype(np.float64))
    for accum in (0.0, 1.0):
        dg, db = dev(prior[0]), dev(prior[1])
        ops.bn_param_grads(dev(y), dev(g), dev(gamma), dev(beta), dg, db, beta=accum)
        rg, rb = dgamma + accum * prior[0], dbeta + accum * prior[1]
        # dbeta: the reduction bound; accumulate: one product-and-add more
        within(host(db), rb, depth * EPS * s_g + EPS * np.abs(rb), "dbeta, accum %g" % accum)
        # dgamma: a term g * (y - beta) carries two more roundings, the sum is divided by gamma once: the reduction
        # bound scaled by 1 / |gamma| — the same bound for gamma = 0.001 (no cancellation is allowed to hide in it)
        within(host(dg), rg, (depth + 2) * EPS * s_gy / ag + EPS * np.abs(dgamma) + EPS * np.abs(rg), "dgamma, accum %g" % accum)
        bits(host(dg)[~nz], (prior[0] if accum else np.zeros(C, f32))[~nz], "dgamma of a zero gamma is reported as 0")


# ------------------------------------------------------------------------------------------------- spatial mean
@pytest.mark.parametrize("C", [2048, 1536, 6])
@pytest.mark.parametrize("HW", [(1, 1), (2, 3), (7, 1), (2, 4), (4, 4), (7, 7), (8, 8)])
def test_spatial_mean_against_float64(ops, HW, C):
    H, W = HW
    N = 5
    rs = np.random.RandomState(H * W + C)
    x = rs.randn(N, H, W, C).astype(f32)
    m, sabs = S.spatial_mean(x)
    # HW terms added in pixel order, one division
    within(host(ops.spatial_mean_fwd(dev(x))), m, H * W * EPS * sabs / (H * W) + EPS * np.abs(m), "spatial mean")
    dy = rs.randn(N, C).astype(f32)
    ref = S.spatial_mean_bwd(dy, x.shape)
    within(host(ops.spatial_mean_bwd(dev(dy), x.shape)), ref, U * np.abs(ref), "spatial mean backward")    # one division
    act = (rs.randn(N, H, W, C) * 4).astype(f32)
    act.reshape(-1)[::5] = 0.0
    act.reshape(-1)[2::5] = 6.0
    for relu6 in (False, True):
        ref = S.spatial_mean_bwd(dy, x.shape, act, relu6)
        got = host(ops.spatial_mean_bwd(dev(dy), x.shape, mask_ref=dev(act), mask6=relu6))
        within(got, ref, U * np.abs(ref), "masked spatial mean backward")
        off = (act <= 0) | ((act >= 6) if relu6 else False)
        assert (got[off] == 0).all() and (got[(act == 6) & (dy[:, None, None, :] != 0)] != 0).all() == (not relu6)


# ------------------------------------------------------------------------------------------------ data movement
def test_copy_channels_at_the_mixed_block_widths(ops):
    """tf.concat / slice at the Inception-ResNet-v2 Mixed_5b (96+64+96+64), Mixed_6a (384+384+320) and Mixed_7a
    (384+288+320+1088) widths; non-zero source AND destination offsets and the accumulate mode through the C entry."""
    from mtl_ssl_amd.lib import lib, ptr
    rs = np.random.RandomState(6)
    for widths, hw in (((96, 64, 96, 64), (13, 21)), ((384, 384, 320), (9, 11)), ((384, 288, 320, 1088), (8, 8))):
        parts = [rs.randn(2, hw[0], hw[1], c).astype(f32) for c in widths]
        cat = np.concatenate(parts, 3)
        got = ops.concat_channels([dev(p) for p in parts])
        bits(host(got), cat, "concat")
        c0 = 0
        for p in parts:
            bits(host(ops.slice_channels(got, c0, p.shape[3])), p, "slice at %d" % c0)
            c0 += p.shape[3]
        C, rows = cat.shape[3], cat.shape[0] * hw[0] * hw[1]
        nc, s0, d0 = widths[1] - 8, widths[0] + 4, 12                              # slice -> slice, both offsets non-zero
        wide = rs.randn(2, hw[0], hw[1], C + 16).astype(f32)
        for acc in (0, 1):
            dst = dev(wide)
            lib().copy_channels(ptr(got), C, s0, ptr(dst), C + 16, d0, rows, nc, acc, ops._stream())
            ref = wide.copy()
            ref[..., d0:d0 + nc] = (wide[..., d0:d0 + nc] * acc + cat[..., s0:s0 + nc]).astype(f32)   # one exact-rounded add
            bits(host(dst), ref, "copy_channels accumulate %d" % acc)


def test_clip_to_window_is_exact(ops):
    rs = np.random.RandomState(8)
    b = (rs.rand(1000, 4) * 3 - 1).astype(f32)
    b[0] = (0.5, 0.5, 0.5, 0.5)                                                    # degenerate, inside
    b[1] = (-3, -3, -2, -2)                                                        # wholly outside: collapses onto the corner
    b[2] = (2, 2, 3, 3)
    b[3] = (0.0, 0.25, 1.0, 0.75)                                                  # the window itself
    for win in ((0.0, 0.0, 1.0, 1.0), (0.0, 0.25, 1.0, 0.75), (-0.5, 0.1, 0.4, 2.0)):
        bits(host(ops.clip_to_window(dev(b), win)), S.clip_to_window(b, win), "clip_to_window")


@pytest.mark.parametrize("n2,n_expand", [(64, 5), (300, 5), (7, 3)])
def test_expand_windows_against_its_fp32_sequence(ops, n2, n_expand):
    rs = np.random.RandomState(n2)
    p = np.sort(rs.rand(2, n2, 2, 2).astype(f32), 2).reshape(2, n2, 4)
    p[0, 0] = (0, 0, 1, 1)
    p[0, 1] = (0.25, 0.5, 0.75, 1.0)
    got = host(ops.expand_windows(dev(p), n_expand))
    bits(got, S.expand_windows_f32(p, n_expand), "expand_windows (glue.hip is built without contraction)")
    # against float64: a division, a product and an addition on values <= 1: three roundings, 3 * eps/2 absolute
    within(got, S.expand_windows(p, n_expand), 3 * U, "expand_windows")
    bits(got[:, 0], p, "window 0 is the proposal")
    # what dedup_windows relies on: the last window is [0, 0, 1, 1] up to the last bit of z + (1 - z)
    z = p[..., 2:]
    bits(got[:, -1, :, 2:], (z + ((f32(1) - z) / f32(n_expand - 1)) * f32(n_expand - 1)).astype(f32), "last window, far corner")
    assert (np.abs(got[:, -1, :, 2:] - 1) <= EPS).all() and (np.abs(got[:, -1, :, :2]) <= EPS).all()
