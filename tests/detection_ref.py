"""Float64 definitions, error bounds and case tables of the detection-kernel edge tests
(tests/detection_edges/test_gpu_detection.py on the device, tests/test_detection_ref.py on the CPU): anchors, window
prune / clip, the Faster R-CNN box coder, IoU + arg-max matching + target assignment, greedy NMS, multiclass NMS and
the score converters of mtl_ssl_amd/csrc/detection.hip. A plain module: no fixtures, not a conftest.

Every definition is written from the reference's formula in numpy float64 (the file and lines are cited per function),
not from the kernel; `mutate=` names one deliberately wrong variant, which test_detection_ref.py uses to show that the
case tables tell the variants apart.

Bounds (the convention of tests/f64_check.py): u = EPS / 2 is the fp32 unit roundoff; data movement and comparisons
are bit-exact; a fixed sequence of r roundings is within r * u of float64, relative to the operands named at each
bound; every bound is multiplied by 1 + 1e-6 for the terms in u^2.

Integer outputs hinge on fp32 comparisons. They are asserted bit for bit against the fp32 oracle (oracle/), and
against the float64 definition everywhere except on KNIFE-EDGE elements:
  * an anchor whose float64 best IoU lies within 4 EPS (relative) of a threshold or of its runner-up;
  * for a forced match, every anchor whose IoU with the groundtruth row lies within 4 EPS of the row's best;
  * for NMS, a candidate whose float64 IoU with an earlier survivor lies within 4 EPS of the threshold: selections are
    compared up to the first such candidate (a flipped decision changes everything after it).
A random case may leave out at most KNIFE_CAP = 0.5 % of its elements this way; the constructed cases use IoUs that
are exact in both precisions (1/4, 1/2, 3/4 from small integer boxes) and leave out none.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)
U = EPS / 2
SLACK = 1.0 + 1e-6
f32 = np.float32
f64 = np.float64
KNIFE = 4 * EPS
KNIFE_CAP = 0.005

# Accuracy of the device logf (the one number of the coder that cannot be derived), handled like TANH_ULPS_MEASURED of
# tests/conv_ref.py. Measured on an MI355X: the worst distance, in fp32 ulps of the float64 logarithm, between th / tw
# divided by their scale factor and log() in float64 of the bit-reproduced fp32 argument (encode_arg32), over every
# case of CODER_KINDS x CODER_SIZES x SCALE_FACTORS (worst: 2.4133, 'ordinary', n = 255, factors (10, 10, 5, 5); 1.8338
# under the factors (1, 1, 1, 1), i.e. logf alone) and every matched anchor of assign_cases() under every pair of
# THRESHOLDS, force on and off (worst: 2.0274). The distance includes the rounding of the scale product. Asserted
# against twice the measured value: the factor covers arguments the cases do not sample. The GPU module prints the
# observed worst beside this number on every run.
LOG_ULPS_MEASURED = 2.4133
LOG_ULPS = 2 * LOG_ULPS_MEASURED

SCALE_FACTORS = ((10.0, 10.0, 5.0, 5.0), (1.0, 1.0, 1.0, 1.0), (2.0, 3.0, 4.0, 7.0))
THRESHOLDS = ((0.75, 0.25), (0.5, 0.5), (0.7, 0.3))


def _b(boxes):
    return np.asarray(boxes, f64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------- box arithmetic
def iou64(boxes1, boxes2):
    """core/box_list_ops.py:203-272 (intersection, iou): [N, M]; 0 where the intersection is 0."""
    a, b = _b(boxes1), _b(boxes2)
    h = np.maximum(0.0, np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]))
    w = np.maximum(0.0, np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]))
    inter = h * w
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
    union = area(a)[:, None] + area(b)[None, :] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(inter == 0, 0.0, inter / union)


def clip64(boxes, window):
    """core/box_list_ops.py:102-137 without the filter: min with the window's max, then max with its min."""
    b = _b(boxes)
    w = np.asarray(window, f64)
    lo, hi = np.array([w[0], w[1], w[0], w[1]]), np.array([w[2], w[3], w[2], w[3]])
    return np.maximum(np.minimum(b, hi), lo)


def prune64(boxes, window):
    """core/box_list_ops.py:140-169: indices of the boxes that lie wholly inside the window (edges included)."""
    b = _b(boxes)
    w = np.asarray(window, f64)
    bad = (b[:, 0] < w[0]) | (b[:, 1] < w[1]) | (b[:, 2] > w[2]) | (b[:, 3] > w[3])
    return np.nonzero(~bad)[0].astype(np.int32)


def change_frame64(boxes, window):
    """core/box_list_ops.py:363-390: (box - window min) scaled by 1 / window extent."""
    b = _b(boxes)
    w = np.asarray(window, f64)
    return (b - np.array([w[0], w[1], w[0], w[1]])) / np.array([w[2] - w[0], w[3] - w[1], w[2] - w[0], w[3] - w[1]])


def change_frame_bound(ref):
    """fp32: the difference, the reciprocal of the extent, the product: 3 roundings relative to the result (the
    extents of the windows in the tables are integers below 2^24: exact)."""
    return 3 * U * np.abs(ref) * SLACK


# ------------------------------------------------------------------------------------------------- anchors
def anchors64(grid_h, grid_w, scales, aspect_ratios, base=(256.0, 256.0), stride=(16.0, 16.0), offset=(0.0, 0.0)):
    """anchor_generators/grid_anchor_generator.py:96-214 (tile_anchors): y outer, x, then aspect-major anchor types;
    h = scale / sqrt(ratio) * base_h, w = scale * sqrt(ratio) * base_w, centre = index * stride + offset. The
    parameters enter as the fp32 numbers the device receives. -> (anchors [n, 4], bound [n, 4]).

    Bound: h (w): root, quotient (product), product by the base: 3u |h|, halved exactly; centre: product (u |i s|) and
    sum (u |c|); corner: one more sum (u |corner|)."""
    sc, ar = np.asarray(scales, f32).astype(f64), np.asarray(aspect_ratios, f32).astype(f64)
    bh, bw, sy, sx, oy, ox = [float(f32(v)) for v in (*base, *stride, *offset)]
    rs = np.sqrt(np.repeat(ar, len(sc)))
    s = np.tile(sc, len(ar))
    h, w = s / rs * bh, s * rs * bw
    iy, ix = np.arange(grid_h, dtype=f64), np.arange(grid_w, dtype=f64)
    shape = (grid_h, grid_w, len(h))
    yc = np.broadcast_to((iy * sy + oy)[:, None, None], shape)
    xc = np.broadcast_to((ix * sx + ox)[None, :, None], shape)
    py = np.broadcast_to(np.abs(iy * sy)[:, None, None], shape)
    px = np.broadcast_to(np.abs(ix * sx)[None, :, None], shape)
    hh, ww = np.broadcast_to(h, shape), np.broadcast_to(w, shape)
    out = np.stack([yc - 0.5 * hh, xc - 0.5 * ww, yc + 0.5 * hh, xc + 0.5 * ww], -1)
    cen = np.stack([py + np.abs(yc), px + np.abs(xc)] * 2, -1)
    half = np.stack([1.5 * np.abs(hh), 1.5 * np.abs(ww)] * 2, -1)
    bound = U * (cen + half + np.abs(out)) * SLACK
    return out.reshape(-1, 4), bound.reshape(-1, 4)


# ------------------------------------------------------------------------------------------------- box coder
EPSILON64 = float(f32(1e-8))      # box_coders/faster_rcnn_box_coder.py:37 (EPSILON = 1e-8), as the fp32 graph holds it


def _center_size64(b):
    """core/box_list.py:158-174."""
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    return b[:, 0] + h / 2, b[:, 1] + w / 2, h, w


def encode64(boxes, anchors, scale_factors=(10.0, 10.0, 5.0, 5.0), mutate=None):
    """box_coders/faster_rcnn_box_coder.py:60-90 -> [n, 4] (ty, tx, th, tw). mutate='no_epsilon' leaves EPSILON out."""
    b, a = _b(boxes), _b(anchors)
    yca, xca, ha, wa = _center_size64(a)
    yc, xc, h, w = _center_size64(b)
    e = 0.0 if mutate == "no_epsilon" else EPSILON64
    ha, wa, h, w = ha + e, wa + e, h + e, w + e
    s = [float(v) for v in scale_factors]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([(yc - yca) / ha * s[0], (xc - xca) / wa * s[1], np.log(h / ha) * s[2], np.log(w / wa) * s[3]], 1)


def encode_arg32(boxes, anchors):
    """The argument of the coder's logarithms, step by step in fp32 as the kernel (and the oracle) evaluate it:
    r = f32(f32(f32(y1 - y0) + 1e-8f) / f32(f32(ya1 - ya0) + 1e-8f)) for h, the same in x for w -> (rh, rw) fp32."""
    b, a = np.asarray(boxes, f32).reshape(-1, 4), np.asarray(anchors, f32).reshape(-1, 4)
    e = f32(1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        rh = ((b[:, 2] - b[:, 0]).astype(f32) + e).astype(f32) / ((a[:, 2] - a[:, 0]).astype(f32) + e).astype(f32)
        rw = ((b[:, 3] - b[:, 1]).astype(f32) + e).astype(f32) / ((a[:, 3] - a[:, 1]).astype(f32) + e).astype(f32)
    return rh.astype(f32), rw.astype(f32)


def encode_center_bound(boxes, anchors, scale_factors):
    """Bound of ty, tx against encode64 -> [n, 2]. fp32 sequence per axis: h = y1 - y0 and ha likewise (u each, halved
    exactly), yc = y0 + h / 2 and yca (u |yc|, u |yca|), d = yc - yca (u |d|): the absolute error of d is
    u (|h| / 2 + |yc| + |ha| / 2 + |yca| + |d|) — relative to the coordinates that cancel, not to d; the denominator
    ha + EPSILON carries 2 roundings, the quotient and the scale one each: 4u |t|."""
    b, a = _b(boxes), _b(anchors)
    out = []
    for ax in (0, 1):
        h, ha = b[:, 2 + ax] - b[:, ax], a[:, 2 + ax] - a[:, ax]
        c, ca = b[:, ax] + h / 2, a[:, ax] + ha / 2
        den = ha + EPSILON64
        s = float(scale_factors[ax])
        d_abs = U * (np.abs(h) / 2 + np.abs(c) + np.abs(ha) / 2 + np.abs(ca) + np.abs(c - ca))
        out.append((s * d_abs / np.abs(den) + 4 * U * np.abs((c - ca) / den * s)) * SLACK)
    return np.stack(out, 1)


def log_distance(got, boxes, anchors, scale_factors):
    """Worst distance in fp32 ulps between th / tw divided by their scale factor and the float64 logarithm of
    encode_arg32 (what LOG_ULPS_MEASURED records); asserts nothing."""
    got = np.asarray(got, f32).reshape(-1, 4).astype(f64)
    worst = 0.0
    for col, r in zip((2, 3), encode_arg32(boxes, anchors)):
        with np.errstate(divide="ignore", invalid="ignore"):
            lr = np.log(r.astype(f64))
        m = np.isfinite(lr)
        if m.any():
            worst = max(worst, float(ulps32(got[m, col] / float(scale_factors[col]), lr[m]).max()))
    return worst


def check_encode(got, oracle_codes, boxes, anchors, scale_factors, what, log_ulps=None):
    """Every assertion on a block of codes (boxes_encode, or the matched rows of reg_targets):
      * ty, tx bit for bit the fp32 sequence of oracle/boxes.py, and within encode_center_bound of encode64;
      * th, tw: |t / s - log(r)| <= LOG_ULPS ulp32(log r) + u |log r| with r = encode_arg32 (the device logf, plus the
        rounding of the scale product), and against encode64 with 5u more on log r (r is 5 roundings from the float64
        ratio: two differences, two sums with EPSILON, the quotient; a relative error of r is an absolute one of log r).
    Rows whose float64 codes are not finite or beyond fp32 range (a zero-size anchor) are compared bitwise with the
    oracle only — the caller does that for all rows anyway. `log_ulps` replaces LOG_ULPS where the logarithm under test
    is not the device's (numpy's, when the oracle itself is checked). -> (worst ulps of the logarithm, worst centre error in
    units of its bound, worst size error in units of its bound)."""
    got = np.asarray(got, f32).reshape(-1, 4)
    ora = np.asarray(oracle_codes, f32).reshape(-1, 4)
    log_ulps = LOG_ULPS if log_ulps is None else log_ulps
    if not len(got):
        return 0.0, 0.0, 0.0
    same = got[:, :2].view(np.int32) == ora[:, :2].view(np.int32)
    assert same.all(), "%s: ty/tx differ from the fp32 sequence at %s" % (what, np.argwhere(~same)[:4].tolist())
    ref = encode64(boxes, anchors, scale_factors)
    ok = np.isfinite(ref).all(1) & (np.abs(ref).max(1) < 1e30)
    g64 = got.astype(f64)
    cb = encode_center_bound(boxes, anchors, scale_factors)
    err_c = np.abs(g64[:, :2] - ref[:, :2])
    bad = ok[:, None] & ~(err_c <= cb)
    assert not bad.any(), "%s: ty/tx out of bound at %s" % (what, np.argwhere(bad)[:4].tolist())
    worst_c = float((err_c[ok] / np.maximum(cb[ok], 1e-300)).max()) if ok.any() else 0.0
    rh, rw = encode_arg32(boxes, anchors)
    worst_u = worst_s = 0.0
    for col, r in ((2, rh), (3, rw)):
        s = float(scale_factors[col])
        with np.errstate(divide="ignore", invalid="ignore"):
            lr = np.log(r.astype(f64))
        m = np.isfinite(lr)
        ulp = np.spacing(np.abs(lr[m]).astype(f32)).astype(f64)
        d = np.abs(g64[m, col] / s - lr[m])
        tol = log_ulps * ulp + U * np.abs(lr[m])
        if m.any():
            worst_u = max(worst_u, float((d / ulp).max()))
        assert (d <= tol).all(), "%s: log column %d: %.3f ulps at row %d" % (
            what, col, float((d / ulp).max()), int(np.nonzero(m)[0][int(np.argmax(d / ulp))]))
        m &= ok
        ulp = np.spacing(np.abs(lr[m]).astype(f32)).astype(f64)
        d64 = np.abs(g64[m, col] - ref[m, col])
        tol64 = (s * (log_ulps * ulp + 5 * U) + U * np.abs(ref[m, col])) * SLACK
        assert (d64 <= tol64).all(), "%s: th/tw column %d against encode64: worst %.3f of its bound" % (
            what, col, float((d64 / tol64).max()))
        if m.any():
            worst_s = max(worst_s, float((d64 / tol64).max()))
    return worst_u, worst_c, worst_s


def decode64(codes, anchors, scale_factors=(10.0, 10.0, 5.0, 5.0)):
    """box_coders/faster_rcnn_box_coder.py:92-118, plain np.exp -> (boxes [n, 4], bound [n, 4]).

    Bound, per axis: ha = y1 - y0 (u |ha|), yca = y0 + ha / 2 (u |ha| / 2 + u |yca|), t = ty / s (u), t * ha (the
    error of t, of ha and the product: 3u |t ha|), yc = t ha + yca (u |yc|); the size: t' = th / s is off by u |t'|,
    which is a relative error of exp(t'); exp_rn is within 2 ulps of a double and is rounded once to fp32 (u), ha
    brings u, the product u: h is within (|t'| + 3) u + 2^-51 relative; h / 2 is exact; the corner is one more sum."""
    c, a = _b(codes), _b(anchors)
    s = [float(v) for v in scale_factors]
    out, bound = [None] * 4, [None] * 4
    for ax in (0, 1):
        ha = a[:, 2 + ax] - a[:, ax]
        ca = a[:, ax] + ha / 2
        t, ts = c[:, ax] / s[ax], c[:, 2 + ax] / s[2 + ax]
        with np.errstate(over="ignore"):
            h = np.exp(ts) * ha
        ctr = t * ha + ca
        e_ctr = U * (3 * np.abs(t * ha) + np.abs(ha) / 2 + np.abs(ca) + np.abs(ctr))
        e_half = 0.5 * np.abs(h) * ((np.abs(ts) + 3) * U + 2.0 ** -51)
        for k, sign in ((ax, -1.0), (2 + ax, 1.0)):
            out[k] = ctr + sign * h / 2
            bound[k] = (e_ctr + e_half + U * np.abs(out[k])) * SLACK
    return np.stack(out, 1), np.stack(bound, 1)


# ------------------------------------------------------------------------------------------------- matcher
MATCH_MUTANTS = ("matched_ge", "unmatched_ge", "col_last", "row_last", "smaller_row_wins")


def _argmax(m, axis, last=False):
    if not last:
        return np.argmax(m, axis)
    return m.shape[axis] - 1 - np.argmax(np.flip(m, axis), axis)


def match64(sim, mthr, uthr, force, mutate=None):
    """matchers/argmax_matcher.py:102-189 with negatives_lower_than_unmatched=True -> int32 [N].

    sim [G, N]. G == 0: every column is -1. Tie rules, stated once:
      * the column arg-max takes the FIRST maximum: of two groundtruth rows with the same IoU on an anchor, the
        smaller row index wins;
      * below = uthr > best gives -1; between = best >= uthr and mthr > best gives -2: a value ON the matched
        threshold is matched, a value ON the unmatched threshold (and below the matched one) is ignored;
      * force: the row arg-max takes the FIRST maximum (the smallest anchor index; a row of zeros forces anchor 0), and
        the forced values are written in row order (dynamic_stitch, :167): LATER rows overwrite earlier ones.
    mutate: one of MATCH_MUTANTS."""
    sim = np.asarray(sim, f64)
    G, N = sim.shape
    if G == 0:
        return np.full(N, -1, np.int32)
    match = _argmax(sim, 0, last=mutate == "col_last").astype(np.int64)
    best = sim.max(0)
    below = (uthr >= best) if mutate == "unmatched_ge" else (uthr > best)
    matched_fail = (mthr >= best) if mutate == "matched_ge" else (mthr > best)
    between = ~below & matched_fail
    match = np.where(below, -1, match)
    match = np.where(between, -2, match)
    if force:
        cols = _argmax(sim, 1, last=mutate == "row_last")
        rows = range(G - 1, -1, -1) if mutate == "smaller_row_wins" else range(G)
        for r in rows:
            match[cols[r]] = r
    return match.astype(np.int32)


def match_knife(sim, mthr, uthr, force):
    """The knife-edge anchors of a similarity matrix (module docstring) -> bool [N]. Exact zeros are no knife edge:
    an empty intersection is empty in both precisions."""
    sim = np.asarray(sim, f64)
    G, N = sim.shape
    knife = np.zeros(N, bool)
    if G == 0:
        return knife
    srt = np.sort(sim, 0)
    best = srt[-1]
    for t in (mthr, uthr):
        knife |= np.abs(best - t) <= KNIFE * t
    if G > 1:
        knife |= (best > 0) & (best - srt[-2] <= KNIFE * best)
    if force:
        rbest = sim.max(1)
        for r in range(G):
            if rbest[r] > 0:
                near = rbest[r] - sim[r] <= KNIFE * rbest[r]
                if near.sum() > 1:
                    knife |= near
    return knife


# ------------------------------------------------------------------------------------------------- NMS
def _nms_iou64(box, others):
    """tf.image.non_max_suppression's IoU (TF 1.7 non_max_suppression_op.cc): corners in either order; a pair with a
    box of no area never suppresses. box [4], others [k, 4] -> (iou [k], valid [k])."""
    def norm(b):
        return (np.minimum(b[..., 0], b[..., 2]), np.minimum(b[..., 1], b[..., 3]),
                np.maximum(b[..., 0], b[..., 2]), np.maximum(b[..., 1], b[..., 3]))
    y0, x0, y1, x1 = norm(box)
    Y0, X0, Y1, X1 = norm(others)
    aa, ab = (y1 - y0) * (x1 - x0), (Y1 - Y0) * (X1 - X0)
    ih = np.maximum(np.minimum(y1, Y1) - np.maximum(y0, Y0), 0.0)
    iw = np.maximum(np.minimum(x1, X1) - np.maximum(x0, X0), 0.0)
    inter = ih * iw
    valid = (aa > 0) & (ab > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(valid, inter / (aa + ab - inter), 0.0)
    return q, valid


def greedy_nms64(boxes, scores, max_out, thr, mutate=None):
    """Greedy NMS as core/post_processing.py:146 calls it: candidates by score descending, equal scores in index order
    (a stable sort: the order this project defines, oracle/nms.py); a candidate survives iff its IoU with every
    earlier survivor is NOT > thr; at most max_out survivors. mutate='iou_ge' suppresses at IoU == thr as well.
    -> (selected int32 [k], `sure`: how many leading entries of `selected` were decided before the first knife-edge
    candidate, n_knife)."""
    b = _b(boxes)
    s = np.asarray(scores, f64).reshape(-1)
    order = np.argsort(-s, kind="stable")
    sel, sure, n_knife = [], None, 0
    for c in order:
        if len(sel) >= max_out:
            break
        keep = True
        if sel:
            q, valid = _nms_iou64(b[c], b[sel])
            hit = valid & ((q >= thr) if mutate == "iou_ge" else (q > thr))
            keep = not hit.any()
            if (valid & (q > 0) & (np.abs(q - thr) <= KNIFE * thr)).any():      # an empty intersection is exact
                n_knife += 1
                if sure is None:
                    sure = len(sel)
        if keep:
            sel.append(int(c))
    return np.asarray(sel, np.int32), (len(sel) if sure is None else sure), n_knife


MERGE_MUTANTS = ("merge_reversed_ties", "merge_unstable")


def multiclass_merge(class_scores, max_total, mutate=None):
    """core/post_processing.py:148-163: concatenate the per-class selections in class order, sort by score descending
    and STABLY (box_list_ops.sort_by_field: ties keep class order, then selection order), cut at max_total.
    class_scores: one array per class -> list of (class, position in the class's selection).
    mutate: 'merge_reversed_ties' (ties in reverse order), 'merge_unstable' (ties by position before class)."""
    items = [(c, k, float(v)) for c, sc in enumerate(class_scores) for k, v in enumerate(sc)]
    if mutate == "merge_reversed_ties":
        items = items[::-1]
    elif mutate == "merge_unstable":
        items.sort(key=lambda t: (t[1], t[0]))
    items.sort(key=lambda t: -t[2])                 # list.sort is stable
    return [(c, k) for c, k, _ in items[:max_total]]


def batch_multiclass_nms64(boxes, scores, score_thresh, iou_thresh, max_per_class, max_total, clip_window=None,
                           change_frame=False, num_valid=None, mutate=None):
    """core/post_processing.py:25-312 in float64. boxes [B, n, q, 4], scores [B, n, C] (fp32 values; they are only
    compared and copied). Per image and class: the first num_valid boxes, score > score_thresh
    (filter_greater_than: strict; mutate='score_ge'), clip_to_window and drop area <= 0, change_coordinate_frame,
    greedy NMS with min(max_per_class, candidates); then multiclass_merge and zero padding.
    -> (boxes [B, T, 4] f64, scores [B, T], classes [B, T], num [B], `sure` [B]: False where a knife-edge NMS
    decision was met in the image, `frame` [B, T]: True where the box went through the change of frame)."""
    boxes, scores = np.asarray(boxes, f64), np.asarray(scores, f64)
    Bn, n, q, _ = boxes.shape
    C = scores.shape[2]
    T = int(max_total)
    ob, os_, oc = np.zeros((Bn, T, 4)), np.zeros((Bn, T)), np.zeros((Bn, T))
    on, sure = np.zeros(Bn, np.int32), np.ones(Bn, bool)
    for i in range(Bn):
        nv = n if num_valid is None else min(int(num_valid[i]), n)
        cb, cs = [], []
        for c in range(C):
            b, s = boxes[i, :nv, c if q > 1 else 0], scores[i, :nv, c]
            keep = (s >= score_thresh) if mutate == "score_ge" else (s > score_thresh)
            b, s = b[keep], s[keep]
            if clip_window is not None:
                b = clip64(b, clip_window)
                keep = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) > 0
                b, s = b[keep], s[keep]
                if change_frame:
                    b = change_frame64(b, clip_window)
            sel, ns, nk = greedy_nms64(b, s, min(max_per_class, len(b)), iou_thresh,
                                       mutate if mutate == "iou_ge" else None)
            sure[i] &= nk == 0
            cb.append(b[sel])
            cs.append(s[sel])
        order = multiclass_merge(cs, T, mutate if mutate in MERGE_MUTANTS else None)
        for t, (c, k) in enumerate(order):
            ob[i, t], os_[i, t], oc[i, t] = cb[c][k], cs[c][k], c
        on[i] = len(order)
    return ob, os_, oc, on, sure


# ------------------------------------------------------------------------------------------------- score converters
def softmax64(x):
    """tf.nn.softmax over the last axis."""
    x = np.asarray(x, f64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def sigmoid64(x):
    """tf.sigmoid."""
    x = np.asarray(x, f64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def ulps32(got, ref):
    """|got - ref| in fp32 ulps of ref (the spacing of the fp32 number nearest to it)."""
    ref = np.asarray(ref, f64)
    return np.abs(np.asarray(got, f64) - ref) / np.spacing(np.abs(ref).astype(f32)).astype(f64)


# ===================================================================================================== case tables
def rand_boxes(rng, n, H=600.0, W=1024.0, min_size=4.0):
    y0, x0 = rng.uniform(-0.1 * H, 0.9 * H, n), rng.uniform(-0.1 * W, 0.9 * W, n)
    h, w = rng.uniform(min_size, 0.6 * H, n), rng.uniform(min_size, 0.6 * W, n)
    return np.stack([y0, x0, y0 + h, x0 + w], 1).astype(f32)


# ---- anchors
ANCHOR_GRIDS = ((1, 1), (1, 257), (3, 5))
ANCHOR_TYPES = {1: ([1.0], [1.0]), 12: ([0.25, 0.5, 1.0, 2.0], [0.5, 1.0, 2.0]),
                64: ([0.1 * (i + 1) for i in range(8)], [0.3 + 0.45 * i for i in range(8)])}
ANCHOR_GEOMETRY = (((256.0, 256.0), (16.0, 16.0), (0.0, 0.0)), ((200.0, 300.0), (8.0, 16.5), (4.0, -3.0)))
ANCHOR_TOO_MANY = ([0.1 * (i + 1) for i in range(13)], [0.5, 1.0, 2.0, 3.0, 4.0])       # 65 types

# ---- prune / clip
PRUNE_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
WINDOWS = ((0.0, 0.0, 600.0, 1024.0), (10.5, -7.0, 333.25, 512.0))


def prune_case(n, window, seed=0):
    """n boxes for the window: random ones (about half inside), flipped ones, boxes wholly outside, and — from index 0
    on, as many as fit — four boxes that touch one window edge each from the inside (kept) and four that are one fp32
    step outside that edge (pruned). -> (boxes [n, 4] fp32, indices of the on-edge boxes, of the one-step-out boxes)."""
    rng = np.random.RandomState(1000 + n + seed)
    wy0, wx0, wy1, wx1 = [f32(v) for v in window]
    H, W = float(wy1 - wy0), float(wx1 - wx0)
    cy, cx = rng.uniform(wy0, wy1, n), rng.uniform(wx0, wx1, n)
    h, w = rng.uniform(1, 0.7 * H, n), rng.uniform(1, 0.7 * W, n)
    b = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(f32)
    if n > 20:
        b[12] = b[12][[2, 3, 0, 1]]                                  # flipped
        b[13] = [wy1 + 5, wx1 + 5, wy1 + 50, wx1 + 60]               # wholly outside
        b[14] = [wy0 - 50, wx0 - 60, wy0 - 5, wx0 - 5]
        b[15] = [wy1 + 50, wx0 - 5, wy0 - 50, wx0 - 60]              # outside and flipped
    inner = np.array([wy0 + f32(0.25) * f32(H), wx0 + f32(0.25) * f32(W), wy1 - f32(0.25) * f32(H), wx1 - f32(0.25) * f32(W)], f32)
    edge = [wy0, wx0, wy1, wx1]
    out = [np.nextafter(wy0, f32(-np.inf)), np.nextafter(wx0, f32(-np.inf)), np.nextafter(wy1, f32(np.inf)),
           np.nextafter(wx1, f32(np.inf))]
    on, off = [], []
    for k in range(4):
        if 2 * k + 1 < n:
            b[2 * k] = inner; b[2 * k, k] = edge[k]; on.append(2 * k)
            b[2 * k + 1] = inner; b[2 * k + 1, k] = out[k]; off.append(2 * k + 1)
    return b, on, off


# ---- gather / scatter
GATHER_BATCH = (1, 3)
GATHER_ROW_LEN = (1, 2, 4, 5, 91)
GATHER_N_IDX = (0, 1, 255, 256, 257)
GATHER_N_SRC = 300

# ---- coder
CODER_SIZES = (1, 255, 256, 257)
CODER_KINDS = ("ordinary", "tiny", "huge", "special")


def coder_case(kind, n, seed=0):
    """(boxes, anchors) [n, 4] fp32. ordinary: image-sized boxes near their anchors; tiny: anchors of size 1e-3; huge:
    anchors of size 1e4; special: ordinary, with row 0 a box EQUAL to its anchor (codes exactly 0) and the last row
    (n > 1) a zero-size anchor, the row before it (n > 2) one whose centre codes overflow to infinity under the scale
    factor 10 (both bitwise against the oracle)."""
    rng = np.random.RandomState(2000 + 7 * n + seed + 100 * CODER_KINDS.index(kind))
    size = {"ordinary": 1.0, "special": 1.0, "tiny": 1e-3 / 300.0, "huge": 1e4 / 300.0}[kind]
    a = rand_boxes(rng, n, 600.0, 1024.0, 8.0).astype(f64)
    ctr = np.stack([(a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2], 1)
    hw = np.stack([a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]], 1) * size
    a = np.concatenate([ctr - hw / 2, ctr + hw / 2], 1)
    bc = ctr + rng.uniform(-0.5, 0.5, (n, 2)) * hw
    bhw = hw * np.exp(rng.uniform(-1, 1, (n, 2)))
    b = np.concatenate([bc - bhw / 2, bc + bhw / 2], 1)
    a, b = a.astype(f32), b.astype(f32)
    if kind == "special":
        b[0] = a[0]
        if n > 1:
            a[-1] = [a[-1, 0], a[-1, 1], a[-1, 0], a[-1, 1]]
        if n > 2:                       # a zero-size anchor and a box 2e30 away: (yc - yca) / 1e-8 = 2e38, times 10 = inf
            a[-2] = 0.0
            b[-2] = [1e30, 1e30, 3e30, 3e30]
    return b, a


def decode_case(kind, batch, n, batched_anchors, seed=0):
    """(codes [batch, n, 4], anchors [n, 4] or [batch, n, 4]) fp32; codes of a trained head's range."""
    rng = np.random.RandomState(3000 + 13 * n + batch + seed)
    anc = np.stack([coder_case(kind, n, seed + 31 * i)[1] for i in range(batch)]) if batched_anchors \
        else coder_case(kind, n, seed)[1]
    codes = (rng.randn(batch, n, 4) * np.array([2.0, 2.0, 1.0, 1.0])).astype(f32)
    codes[0, 0] = 0.0                                                # decodes to the anchor itself
    return codes, anc


# ---- target assignment
def _cell(i, h=4.0, w=4.0, dy=0.0):
    """Anchor / box of the constructed cases: cell i of a row of disjoint 4 x 4 cells, 8 apart in x; small integers, so
    that every area, intersection and union below is exact in fp32."""
    return [dy, 8.0 * i, dy + h, 8.0 * i + w]


def _pad_gt(rows, max_gt):
    g = np.full((max_gt, 4), np.nan, f32)
    g[:len(rows)] = np.asarray(rows, f32).reshape(-1, 4)
    return g


def _labels(rng, B, max_gt, num_gt, d):
    if d == 1:
        return None
    lab = np.full((B, max_gt, d), np.nan, f32)
    for b in range(B):
        g = int(num_gt[b])
        lab[b, :g] = 0.0
        lab[b, np.arange(g), rng.randint(1, d, g)] = 1.0
    return lab


def _extra(rng, B, max_gt, num_gt, e):
    if not e:
        return None
    x = np.full((B, max_gt, e), np.nan, f32)
    for b in range(B):
        x[b, :int(num_gt[b])] = rng.rand(int(num_gt[b]), e).astype(f32)
    return x


# Heights one small step off 3, 2 and 1: with the 4 x 4 anchor (area 16) the box area 4 h, the sum 16 + 4 h and the
# quotient 4 h / 16 are all fp32 numbers for h = 3 +- 2^-20, 2 +- 2^-20 and 1 +- 2^-21 (16 + 4 h needs 24 bits down to
# 2^-19), so the IoU is exact in both precisions and 4 to 8 fp32 steps away from the threshold
STEP = 2.0 ** -20


def constructed_assign_cases():
    """The edge cases of target assignment, each a dict like the random ones plus `edge`: what
    tests/test_detection_ref.py asserts the case to hit. All IoUs are k / 16 of small integers, or one fp32 step off."""
    rng = np.random.RandomState(5)
    cases = []

    def add(name, anchors, gts, edge, d=1, e=0, max_gt=None, **kw):
        gts = [np.asarray(g, f32).reshape(-1, 4) for g in gts]
        mg = max_gt or max(1, max(len(g) for g in gts))
        num = np.array([len(g) for g in gts], np.int32)
        anchors = np.asarray(anchors, f32)
        cases.append(dict(name=name, anchors=anchors, gt=np.stack([_pad_gt(g, mg) for g in gts]), num_gt=num,
                          labels=_labels(rng, len(gts), mg, num, d), extra=_extra(rng, len(gts), mg, num, e),
                          constructed=True, edge=dict(edge, **kw)))

    # IoU on, one step above and one step below 3/4, 1/2 and 1/4: a box of height k (+- 2^-20) on a 4 x 4 anchor
    anchors = [_cell(i) for i in range(10)]
    hs = [3.0, 3.0 + STEP, 3.0 - STEP, 2.0, 2.0 + STEP, 2.0 - STEP, 1.0, 1.0 + STEP / 2, 1.0 - STEP / 2]
    gts = [_cell(i, h=h) for i, h in enumerate(hs)]
    add("thresholds", anchors, [gts], dict(kind="threshold", on={0: 0.75, 3: 0.5, 6: 0.25}), d=2)
    # duplicate groundtruth boxes: anchor 2 ties between rows 1 and 2 (first wins); both rows force anchor 2 (last wins)
    anchors = [_cell(i) for i in range(65)]
    add("duplicate_gt", anchors, [[_cell(7, h=3), _cell(2, h=2), _cell(2, h=2), _cell(64, h=3)]],
        dict(kind="same_column", rows=(1, 2), col=2), d=21, e=21)
    # one box tied on two anchors (IoU 1/2 each: the box is the union of two adjacent 4 x 4 anchors), at the three
    # levels of the row arg-max: inside a wave, across the waves of a 256-anchor block, across blocks
    for name, n, (p, q) in (("tie_wave", 257, (5, 41)), ("tie_block", 257, (70, 200)), ("tie_grid", 513, (100, 300)),
                            ("tie_grid_last_block", 513, (3, 512))):
        anchors = np.array([_cell(i) for i in range(n)], f32)
        X = 8.0 * (n + 4)
        anchors[p], anchors[q] = [0, X, 4, X + 4], [0, X + 4, 4, X + 8]
        add(name, anchors, [[_cell(1, h=3), [0, X, 4, X + 8], _cell(2, h=3)]],
            dict(kind="row_tie", row=1, cols=(p, q)))
    # two and three DIFFERENT rows forcing one column: the column arg-max prefers row 0 (3/4), the forced value is the
    # last row
    anchors = [_cell(i) for i in range(64)]
    add("two_rows_one_column", anchors, [[_cell(9, h=3), _cell(9, h=2)]], dict(kind="same_column", rows=(0, 1), col=9), d=91)
    add("three_rows_one_column", anchors, [[_cell(9, h=3), _cell(9, h=2), _cell(9, h=1), _cell(63, h=3)]],
        dict(kind="same_column", rows=(0, 1, 2), col=9), max_gt=5)
    # a groundtruth box that overlaps nothing: its row of zeros forces anchor 0 — alone, before and after a row that
    # forces anchor 0 with a real overlap
    far = _cell(3, dy=100.0)
    add("gt_overlaps_nothing", anchors, [[far]], dict(kind="zero_row", rows=(0,)))
    add("zero_row_then_real_row_on_anchor_0", anchors, [[far, _cell(0, h=3)]], dict(kind="zero_row", rows=(0,), also=1))
    add("real_row_on_anchor_0_then_zero_row", anchors, [[_cell(0, h=3), far]], dict(kind="zero_row", rows=(1,), also=0))
    # zero-area groundtruth boxes (rows of zeros) and zero-area anchors (columns of zeros), with an ordinary pair
    anchors = [_cell(i) for i in range(63)]
    anchors[5] = _cell(5, h=0)
    anchors[6] = _cell(6, w=0)
    add("zero_area", anchors, [[_cell(2, h=3), _cell(5, h=0), _cell(6, h=2), _cell(7, w=0)]],
        dict(kind="zero_row", rows=(1, 2, 3)), d=2, e=21)
    # per-image anchors (anchors_batched = 1): image 1 sees image 0's anchors in reverse order; image 2 has no box
    a0 = np.array([_cell(i) for i in range(65)], f32)
    g = [_cell(4, h=3), _cell(60, h=2), _cell(61, h=1)]
    add("anchors_per_image", np.stack([a0, a0[::-1].copy(), a0]), [g, g, []], dict(kind="batched"), d=21)
    return cases


ASSIGN_RANDOM = (
    # n, B, max_gt, num_gt per image, label_dim, extra_dim, batched anchors
    (1, 1, 1, (1,), 1, 0, False),
    (63, 1, 1, (0,), 1, 0, False),
    (64, 4, 5, (5, 0, 2, 1), 2, 0, False),
    (65, 1, 5, (2,), 21, 21, False),
    (255, 4, 5, (0, 5, 1, 2), 91, 0, True),
    (256, 1, 256, (256,), 1, 0, False),
    (257, 4, 256, (256, 2, 0, 1), 21, 21, False),
    (513, 1, 1024, (1024,), 2, 0, False),
    (513, 4, 5, (5, 1, 0, 2), 1, 0, False),
    (257, 1, 1024, (2,), 91, 21, False),
)


def random_assign_cases():
    cases = []
    for k, (n, B, max_gt, num, d, e, batched) in enumerate(ASSIGN_RANDOM):
        rng = np.random.RandomState(7000 + k)
        anchors = np.stack([rand_boxes(rng, n, min_size=16.0) for _ in range(B if batched else 1)])
        gts = []
        for b in range(B):
            src = anchors[b if batched else 0][rng.randint(0, n, num[b])].astype(f64)
            size = np.concatenate([src[:, 2:] - src[:, :2]] * 2, 1)
            gts.append(_pad_gt((src + rng.uniform(-0.25, 0.25, src.shape) * size).astype(f32), max_gt))
        num = np.array(num, np.int32)
        cases.append(dict(name="random_n%d_B%d_maxgt%d_%d" % (n, B, max_gt, k), anchors=anchors if batched else anchors[0],
                          gt=np.stack(gts), num_gt=num, labels=_labels(rng, B, max_gt, num, d),
                          extra=_extra(rng, B, max_gt, num, e), constructed=False, edge=None))
    return cases


def assign_cases():
    return constructed_assign_cases() + random_assign_cases()


def case_anchors(case, b):
    return case["anchors"][b] if case["anchors"].ndim == 3 else case["anchors"]


def check_match(match, case, b, mthr, uthr, force, what):
    """One image's match vector against match64, knife-edge anchors left out (none in a constructed case, at most
    KNIFE_CAP of the anchors in a random one) -> number of anchors left out."""
    G = int(case["num_gt"][b])
    anchors = case_anchors(case, b)
    sim = iou64(case["gt"][b, :G], anchors)
    ref = match64(sim, mthr, uthr, force)
    knife = np.zeros(len(anchors), bool) if case["constructed"] else match_knife(sim, mthr, uthr, force)
    assert knife.sum() <= KNIFE_CAP * len(anchors), "%s: %d knife-edge anchors of %d" % (what, knife.sum(), len(anchors))
    bad = (np.asarray(match) != ref) & ~knife
    assert not bad.any(), "%s: match differs from match64 at anchors %s: %s vs %s" % (
        what, np.nonzero(bad)[0][:8].tolist(), np.asarray(match)[bad][:8].tolist(), ref[bad][:8].tolist())
    return int(knife.sum())


def check_nms(selected, boxes, scores, max_out, thr, constructed, what):
    """A selection against greedy_nms64: entry for entry up to the first knife-edge candidate. In a constructed case
    the whole selection is compared: the IoUs it has ON the threshold are exact in both precisions.
    -> number of knife-edge candidates."""
    ref, sure, nk = greedy_nms64(boxes, scores, max_out, thr)
    selected = np.asarray(selected)
    if constructed:
        sure = len(ref)
    else:
        assert nk <= KNIFE_CAP * max(len(boxes), 1), "%s: %d knife-edge candidates of %d" % (what, nk, len(boxes))
    if sure == len(ref):
        assert len(selected) == len(ref), "%s: %d selected, float64 selects %d" % (what, len(selected), len(ref))
    assert selected[:sure].tolist() == ref[:sure].tolist(), "%s: selection differs from greedy_nms64" % what
    return 0 if constructed else nk


def check_mc(got, case, what):
    """(boxes, scores, classes, num) of a multiclass NMS against batch_multiclass_nms64: counts, classes and scores
    equal. A random case must meet no knife-edge NMS decision at all (stricter than KNIFE_CAP; its seed is chosen so);
    a constructed one meets IoUs exactly on the threshold, which are exact in both precisions. Boxes bit for bit where
    only clipping acted, within change_frame_bound otherwise -> worst box error in units of the bound."""
    C, c0 = case["C"], case["col0"]
    ref = batch_multiclass_nms64(case["boxes"], case["scores"][:, :, c0:c0 + C], case["score_thresh"], case["iou"], case["mpc"],
                                 case["max_total"], case["window"], case["frame"], case["num_valid"])
    assert case["constructed"] or ref[4].all(), "%s: a knife-edge NMS decision in images %s" % (
        what, np.nonzero(~ref[4])[0].tolist())
    gb, gs, gc, gn = [np.asarray(g) for g in got]
    assert gn.tolist() == ref[3].tolist(), "%s: counts %s, float64 %s" % (what, gn.tolist(), ref[3].tolist())
    assert (gc.astype(f64) == ref[2]).all(), "%s: classes differ" % what
    assert (gs.astype(f64) == ref[1]).all(), "%s: scores differ" % what
    if not case["frame"]:
        assert (gb.astype(f64) == ref[0]).all(), "%s: boxes differ (clipping is exact)" % what
        return 0.0
    tol = change_frame_bound(ref[0])
    err = np.abs(gb.astype(f64) - ref[0])
    assert (err <= tol).all(), "%s: boxes beyond 3 roundings of change_frame64: worst %.2f" % (
        what, float((err / np.maximum(tol, 1e-300)).max()))
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def unmatched_target(d):
    """The unmatched class target: background one-hot for a label row, 0 for the RPN's single column."""
    u = np.zeros(d, f32)
    if d > 1:
        u[0] = 1.0
    return u


# ---- greedy NMS
NMS_SIZES = (0, 1, 2, 64, 65, 129, 300)
NMS_THRESHOLDS = (0.0, 0.5, 1.0)
NMS_MAX_OUT_LIMIT = 4096


def nms_constructed():
    """Boxes whose pairwise IoUs are exact: A and its half B (IoU exactly 1/2: not suppressed at 0.5), a copy of A with
    another score, A with its corners flipped, a zero-area box inside A, and F with G (IoU 3/4) away from the rest."""
    boxes = np.array([[0, 0, 4, 4], [0, 0, 4, 2], [0, 0, 4, 4], [4, 4, 0, 0], [1, 1, 1, 3], [20, 20, 24, 24],
                      [20, 20, 24, 23], [2, 2, 2, 2], [40, 40, 44, 44], [40, 42, 44, 46]], f32)
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.95, 0.2, 0.1], f32)
    return boxes, scores


def nms_case(n, seed=0):
    """n candidates: clustered random boxes with some tied scores, a zero-area box and a flipped box among them
    (identical boxes, whose IoU of exactly 1 sits on the threshold 1.0, are in nms_constructed)."""
    rng = np.random.RandomState(4000 + n + seed)
    if n == 0:
        return np.zeros((0, 4), f32), np.zeros((0,), f32)
    clusters = max(1, n // 6)
    k = rng.randint(0, clusters, n)
    cy, cx = rng.uniform(50, 550, clusters)[k] + rng.normal(0, 6, n), rng.uniform(50, 950, clusters)[k] + rng.normal(0, 6, n)
    h, w = rng.uniform(30, 150, clusters)[k] + rng.normal(0, 4, n), rng.uniform(30, 150, clusters)[k] + rng.normal(0, 4, n)
    b = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1).astype(f32)
    s = ((rng.permutation(n) + 1) / f32(n)).astype(f32)
    if n >= 64:
        s[rng.randint(0, n, n // 8)] = s[1]                   # ties: index order
        b[10] = [b[10, 0], b[10, 1], b[10, 0], b[10, 3]]      # zero area
        b[20] = b[20][[2, 3, 0, 1]]                           # flipped
    return b, s


def nms_cases():
    """(name, boxes, scores, max_out, thr, constructed)"""
    out = []
    cb, cs = nms_constructed()
    for thr in NMS_THRESHOLDS:
        out.append(("constructed_thr%g" % thr, cb, cs, len(cb), thr, True))
    out.append(("constructed_max1", cb, cs, 1, 0.5, True))
    for n in NMS_SIZES:
        b, s = nms_case(n)
        for max_out in sorted({1, max(n, 1), NMS_MAX_OUT_LIMIT}):
            for thr in NMS_THRESHOLDS:
                out.append(("n%d_max%d_thr%g" % (n, max_out, thr), b, s, max_out, thr, False))
    b, s = nms_case(65)
    for max_out in (3072, 3073):        # the largest max_out whose selected boxes the greedy kernel keeps in LDS, and the next
        out.append(("n65_max%d_thr0.5" % max_out, b, s, max_out, 0.5, False))
    return out


# ---- batch multiclass NMS
MC_WINDOWS = ((0.0, 0.0, 256.0, 512.0), (10.0, 20.0, 410.0, 820.0))
MC_SCORE_THRESH = 0.25            # a multiple of 1/16: scores equal to it occur in every case and are filtered out

#            name, B, n, C, q_per_class, col0, num_valid, window index or None, frame, mpc, max_total, iou
MC_TABLE = (
    ("one_box", 1, 1, 1, False, 0, None, None, False, 4, 4, 0.5),
    ("one_class_window", 1, 64, 1, False, 0, (64,), 0, False, 10, 300, 0.5),
    ("two_classes_frame", 3, 65, 2, True, 0, (0, 1, 70), 0, True, 5, 7, 0.5),
    ("offset_window", 3, 64, 2, False, 1, (64, 33, 69), 1, False, 100, 20, 0.5),
    ("offset_window_frame", 1, 300, 2, True, 0, None, 1, True, 20, 30, 0.5),
    ("ninety_classes", 1, 64, 90, True, 1, (60,), 0, True, 3, 100, 0.5),
    ("ninety_classes_shared_boxes", 3, 64, 90, False, 0, (64, 0, 1), 1, True, 2, 500, 0.5),
    ("no_window", 1, 65, 2, True, 0, None, None, False, 4, 5, 0.5),
    ("classes_at_the_limit", 1, 8, 1024, False, 0, None, 0, False, 2, 100, 0.5),
    ("classes_at_the_limit_no_cut", 1, 8, 1024, False, 0, (8,), None, False, 2, 4096, 0.5),
)


def mc_case(row):
    name, B, n, C, qpc, col0, nv, win, frame, mpc, T, iou = row
    rng = np.random.RandomState(6000 + sum(map(ord, name)))
    q = C if qpc else 1
    H, W = (256.0, 512.0) if win is None else (MC_WINDOWS[win][2] + 20.0, MC_WINDOWS[win][3] + 20.0)
    cy, cx = rng.randint(-20, int(H), (B, n, q)), rng.randint(-20, int(W), (B, n, q))
    h, w = rng.randint(4, 120, (B, n, q)), rng.randint(4, 120, (B, n, q))
    boxes = np.stack([cy, cx, cy + h, cx + w], -1).astype(f32)            # integer corners: exact areas and IoUs
    if n > 8:
        boxes[:, 5] = boxes[:, 4]                                          # duplicates
        boxes[:, 6] = np.array([H + 30, W + 30, H + 60, W + 60], f32)      # clips to nothing where a window is set
        boxes[:, 7, :, 2] = boxes[:, 7, :, 0]                              # zero area
    scores = (rng.randint(0, 17, (B, n, C + col0)) / 16.0).astype(f32)     # multiples of 1/16: classes tie
    return dict(name=name, boxes=boxes, scores=scores, col0=col0, C=C, num_valid=None if nv is None else np.array(nv, np.int32),
                window=None if win is None else MC_WINDOWS[win], frame=frame, mpc=mpc, max_total=T, iou=iou,
                score_thresh=MC_SCORE_THRESH, constructed=False)


def mc_cross_class_tie():
    """Three classes share four disjoint boxes; boxes 0 and 1 score 1/2 in every class, box 2 scores exactly the
    threshold, box 3 scores 3/4 in class 1 only. Merged: (1, box 3), then six candidates tied at 1/2 in class order —
    and max_total = 4 cuts inside that group after (0, box 0), (0, box 1), (1, box 0)."""
    boxes = np.array([[[[0, 0, 10, 10]], [[20, 20, 30, 30]], [[40, 40, 50, 50]], [[60, 60, 70, 70]]]], f32)
    scores = np.zeros((1, 4, 3), f32)
    scores[0, :2] = 0.5
    scores[0, 2] = MC_SCORE_THRESH
    scores[0, 3, 1] = 0.75
    return dict(name="cross_class_tie", boxes=boxes, scores=scores, col0=0, C=3, num_valid=None, window=None, frame=False,
                mpc=4, max_total=4, iou=0.5, score_thresh=MC_SCORE_THRESH, constructed=True)


def mc_iou_on_threshold():
    """Two images of the exact pairs of nms_constructed as one class inside a window that clips nothing: IoU 1/2 at
    threshold 1/2 suppresses nothing."""
    cb, cs = nms_constructed()
    boxes = np.stack([cb, cb[::-1]])[:, :, None, :].copy()
    scores = np.stack([cs, cs[::-1]])[:, :, None].copy()
    return dict(name="iou_on_threshold", boxes=boxes, scores=scores, col0=0, C=1, num_valid=None, window=(0.0, 0.0, 64.0, 64.0),
                frame=False, mpc=10, max_total=10, iou=0.5, score_thresh=0.0, constructed=True)


def mc_cases():
    return [mc_cross_class_tie(), mc_iou_on_threshold()] + [mc_case(r) for r in MC_TABLE]


# ---- score converters
SCORE_C = (1, 2, 91)
SCORE_ROWS = (1, 255, 256, 257)


def score_case(rows, C):
    rng = np.random.RandomState(8000 + rows + C)
    x = rng.randn(rows, C) * np.where(rng.rand(rows, 1) < 0.2, 30.0, 3.0)
    return x.astype(f32)
