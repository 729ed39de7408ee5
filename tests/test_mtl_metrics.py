"""CPU checks of the evaluator's multi-task metrics (mtl_ssl_amd/mtl_metrics.py) and of the numpy restatements the GPU
tests hold the new evaluation kernels to: the per-class NMS of the evaluator (against the reference's own
np_box_list_ops outputs, tests/golden/eval_nms_golden.npz) and the edge-mask resize of scikit-image 0.13 / 0.14."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMS_TYPES = {1: "standard", 2: "soft-linear", 3: "soft-gaussian"}


# ------------------------------------------------------------------ numpy restatements (shared with the GPU tests)
def _iou_row(a, b):
    """np_box_ops.iou([a], b)[0] in float64."""
    ih = np.maximum(0.0, np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
    iw = np.maximum(0.0, np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
    inter = ih * iw
    area1 = (a[2] - a[0]) * (a[3] - a[1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area1 + area2 - inter)


def eval_nms_numpy(boxes, scores, scale, nms_type, iou_threshold, sigma, max_output, exp=np.exp):
    """np_box_list_ops.non_max_suppression / soft_non_max_suppression as the evaluator calls them, on fp32 boxes
    promoted to float64 and scaled, fp32 scores. Equal scores sort the later input first (np.argsort(kind="stable")
    reversed), the rule of mtlssl_eval_nms. -> (input indices in output order, fp32 scores)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4).astype(np.float64) * np.broadcast_to(np.asarray(scale, np.float64), (4,))
    s = np.asarray(scores, np.float32).copy()
    keep = np.flatnonzero(s > -10.0)
    src = keep[np.argsort(s[keep], kind="stable")[::-1]]
    b, s = b[src], s[src]
    m = len(src)
    if iou_threshold == 1.0:
        return src[:max_output], s[:max_output]
    valid = np.ones(m, bool)
    if nms_type == "standard":
        sel = []
        for p in range(m):
            if len(sel) >= max_output:
                break
            if not valid[p]:
                continue
            sel.append(p)
            valid[p] = False
            q = np.flatnonzero(valid)
            if q.size:
                with np.errstate(invalid="ignore", divide="ignore"):
                    valid[q] &= _iou_row(b[p], b[q]) <= iou_threshold
        sel = np.asarray(sel, np.int64)
        return src[sel], s[sel]
    selected = 0
    for _ in range(m):
        if selected >= max_output:
            break
        cand = np.flatnonzero(valid & (s > -10.0))
        if not cand.size:
            break
        best = cand[np.argmax(s[cand])]                 # the first maximum
        selected += 1
        valid[best] = False
        q = np.flatnonzero(valid)
        if not q.size:
            break
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = _iou_row(b[best], b[q])
        if nms_type == "soft-linear":
            iou[iou < iou_threshold] = 0
            w = 1 - iou
        else:
            w = exp(-np.square(iou) / sigma)
        s[q] = s[q] * w
    pos = np.flatnonzero(s > 0.0)
    pos = pos[np.argsort(s[pos], kind="stable")[::-1]][:max_output]
    return src[pos], s[pos]


def edgemask_labels_numpy(logits, h, w):
    """skimage.transform.resize(logits, (h, w, 2)) at order 1, mode='constant', cval=0 (scikit-image 0.13 / 0.14),
    .astype(np.float32), then ch0 < ch1 as float32 labels [h,w]."""
    x = np.asarray(logits, np.float32)
    Hf, Wf, _ = x.shape
    rin = (np.arange(h, dtype=np.float64)[:, None] + 0.5) * Hf / h - 0.5
    cin = (np.arange(w, dtype=np.float64)[None, :] + 0.5) * Wf / w - 0.5
    rin, cin = np.broadcast_arrays(rin, cin)
    minr, minc, maxr, maxc = np.floor(rin), np.floor(cin), np.ceil(rin), np.ceil(cin)
    dr, dc = rin - minr, cin - minc

    def px(r, c, ch):
        inside = (r >= 0) & (r < Hf) & (c >= 0) & (c < Wf)
        v = x[np.clip(r, 0, Hf - 1).astype(int), np.clip(c, 0, Wf - 1).astype(int), ch].astype(np.float64)
        return np.where(inside, v, 0.0)

    v = []
    for ch in range(2):
        top = (1 - dc) * px(minr, minc, ch) + dc * px(minr, maxc, ch)
        bot = (1 - dc) * px(maxr, minc, ch) + dc * px(maxr, maxc, ch)
        v.append(((1 - dr) * top + dr * bot).astype(np.float32))
    return (v[0] < v[1]).astype(np.float32)


def portable_exp(x):
    from oracle.portable_math import exp_rn
    return exp_rn(x)


# ------------------------------------------------------------------ the NMS restatement against the reference
def _golden_cases():
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_nms_golden.npz"))
    for i, (t, thr, sigma, cap) in enumerate(g["cases"]):
        yield (i, NMS_TYPES[int(t)], float(thr), float(sigma), int(cap), g["c%d_boxes" % i], g["c%d_scores" % i],
               g["c%d_scale" % i], g["c%d_index" % i], g["c%d_out" % i])


def test_golden_covers_every_type_threshold_and_cap():
    cases = list(_golden_cases())
    assert {c[1] for c in cases} == set(NMS_TYPES.values())
    assert {c[2] for c in cases} >= {0.3, 0.5, 0.7, 1.0}
    assert {c[4] for c in cases} >= {256, 10000}
    # the caps bind somewhere, and soft-NMS drops or reorders something somewhere
    assert any(len(c[8]) == c[4] < len(c[6]) for c in cases)
    assert any(c[1] != "standard" and c[2] < 1.0 and not np.array_equal(c[7], c[6][c[8]]) for c in cases)


def test_numpy_eval_nms_equals_the_reference_outputs():
    for i, t, thr, sigma, cap, boxes, scores, scale, want_i, want_s in _golden_cases():
        got_i, got_s = eval_nms_numpy(boxes, scores, scale, t, thr, sigma, cap)
        assert np.array_equal(got_i, want_i), (i, t, thr, cap)
        assert got_s.dtype == np.float32 and np.array_equal(got_s, want_s), (i, t, thr, cap)


def test_portable_exp_restatement_within_one_ulp_of_the_reference():
    """The device kernel's Gaussian weight uses the portable exponential; against numpy's exp the kept indices are the
    same and every rescored score is within 1 fp32 ulp."""
    n_gauss = 0
    for i, t, thr, sigma, cap, boxes, scores, scale, want_i, want_s in _golden_cases():
        got_i, got_s = eval_nms_numpy(boxes, scores, scale, t, thr, sigma, cap, exp=portable_exp)
        assert np.array_equal(got_i, want_i), (i, t, thr, cap)
        ulps = np.abs(got_s.view(np.int32).astype(np.int64) - want_s.view(np.int32).astype(np.int64))
        assert ulps.max(initial=0) <= (1 if t == "soft-gaussian" else 0), (i, t, int(ulps.max()))
        n_gauss += t == "soft-gaussian"
    assert n_gauss > 0


def test_unknown_nms_type_is_a_value_error():
    from mtl_ssl_amd import config, eval as ev, ops
    cfg = config.parse_pipeline_config('eval_config { nms_type: "soft-cubic" }')
    with pytest.raises(ValueError, match="soft-cubic"):
        ev.eval_nms_options(cfg.eval_config)
    with pytest.raises(ValueError, match="Cannot identify NMS type"):
        ops.eval_nms(None, None, [], "hard", 0.5, 0.5, 100)


def test_eval_nms_options_are_the_protos_float32_values():
    from mtl_ssl_amd import config, eval as ev
    cfg = config.parse_pipeline_config('eval_config { nms_type: "soft-gaussian" nms_threshold: 0.3 '
                                       'soft_nms_sigma: 0.1 iou_threshold: 0.7 }')
    assert ev.eval_nms_options(cfg.eval_config) == ("soft-gaussian", float(np.float32(0.3)), float(np.float32(0.1)),
                                                    float(np.float32(0.7)))
    assert ev.eval_nms_options(config.Msg("EvalConfig")) == ("standard", 1.0, 0.5, 0.5)


# ------------------------------------------------------------------ known answers of the three metrics
def test_window_map_known_answer():
    from mtl_ssl_amd import mtl_metrics
    mm = mtl_metrics.MtlMetrics()
    # image 1: window a ranks both positives first (AP 1), window b ranks its only positive last (AP 1/3)
    mm.add_window(np.float32([[0, 1, 2], [2, 1, 0]]), np.float32([[0, .3, .7], [0, 0, 1]]))
    mm.add_window(np.float32([[0, 5, 0]]), np.float32([[0, 1, 0]]))          # image 2: AP 1
    mm.add_window(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))  # image 3: no windows, skipped
    assert mm.evaluate() == {"mtl/window_map": pytest.approx((2 / 3 + 1) / 2, abs=1e-12)}


def test_closeness_diff_known_answer_with_the_slot_quirk():
    from mtl_ssl_amd import mtl_metrics
    dets = np.float32([[0, 0, 10, 10], [20, 20, 40, 40], [0, 0, 0, 0], [0, 0, 0, 0]])     # padded slots
    gt = np.float32([[22, 22, 38, 38],          # largest intersection with slot 1
                     [100, 100, 110, 110],      # intersects nothing: slot 0
                     [0, 0, 5, 5]])             # label all zero: skipped
    assert list(mtl_metrics.closeness_slots(gt, dets)) == [1, 0, 0]
    # per-PROPOSAL rows, indexed by the detection slot: row 1 says class 2, row 0 says class 1
    logits = np.float32([[0, 5, -5], [0, -5, 5], [0, 9, 9], [0, 0, 0], [0, 0, 0]])
    labels = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 0]])
    mm = mtl_metrics.MtlMetrics()
    mm.add_closeness(logits, labels, gt, dets)          # slot 1 hit, slot 0 miss -> 0.5
    mm.add_closeness(logits, np.float32([[0, 0, 0]]), gt[:1], dets)    # no rows: not in the mean
    mm.add_closeness(logits, np.float32([[0, 1, 0]]), gt[1:2], dets)   # index-0 case: row 0 says class 1 -> hit
    assert mm.evaluate() == {"mtl/closeness_diff": 0.75}
    with pytest.raises(ValueError, match="max_total_detections.*first_stage_max_proposals"):
        mtl_metrics.MtlMetrics().add_closeness(logits[:1], labels, gt, dets)


def test_edgemask_ap_known_answer():
    from mtl_ssl_amd import mtl_metrics
    mm = mtl_metrics.MtlMetrics()
    mm.add_edgemask(6, 2, 4)
    mm.add_edgemask(4, 2, 2)
    assert mm.evaluate() == {"mtl/edgemask_ap": 0.875}
    assert mtl_metrics.MtlMetrics().evaluate() == {}


def test_edgemask_resize_known_answer_constant_not_edge():
    """A 1x1 map whose channel 1 is the smallest fp32 subnormal above channel 0 = 0, resized to 4x4. Output row r
    samples input row (r + 0.5) / 4 - 0.5: rows 0 and 3 take 0.625 of the map and 0.375 of the zero outside it, rows 1
    and 2 take 0.875. A pixel keeps ch1 > ch0 only where its weight w_r * w_c rounds the subnormal to itself (> 0.5);
    with mode='edge' every pixel would read the full value and be labelled 1."""
    tiny = np.float32(1e-45)
    assert tiny > 0
    lab = edgemask_labels_numpy(np.float32([[[0.0, tiny]]]), 4, 4)
    w = np.float64([0.625, 0.875, 0.875, 0.625])
    assert np.array_equal(lab, (np.outer(w, w) > 0.5).astype(np.float32))
    assert lab.sum() == 12 and lab[0, 0] == 0 and lab[1, 1] == 1
    # ordinary values: up / down scaling with non-integer ratios keeps the half-pixel centre rule
    x = np.zeros((2, 3, 2), np.float32)
    x[..., 1] = np.float32([[1, -1, 1], [-1, 1, -1]])
    assert np.array_equal(edgemask_labels_numpy(x, 2, 3), (x[..., 1] > 0).astype(np.float32))
    down = edgemask_labels_numpy(np.repeat(np.repeat(x, 3, 0), 3, 1), 2, 3)
    assert np.array_equal(down, (x[..., 1] > 0).astype(np.float32))
    # a 1x1 output samples the centre of the map
    c = np.zeros((3, 5, 2), np.float32)
    c[1, 2, 1] = 1
    assert edgemask_labels_numpy(c, 1, 1)[0, 0] == 1
