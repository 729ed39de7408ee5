"""The kernels of csrc/detection.hip at their edges, against the float64 definitions of tests/detection_ref.py and, bit
for bit, against the fp32 oracle (oracle/boxes.py, assign.py, nms.py, portable_math.py): anchors, window prune and
clip, row gather / scatter, the box coder, target assignment (thresholds met exactly, ties at every level of the
arg-max reductions, rows forcing one column), greedy NMS under both MTLSSL_NMS_ALGO values, batch multiclass NMS and
the score converters. Every case is small (at most 2 100 boxes); every index handed to a kernel is in range; every
refusal asserted here is a MTLSSL_REQUIRE that returns before any launch. The cases, the bounds and their derivations
are in tests/detection_ref.py; tests/test_detection_ref.py checks them on the CPU.

The module shares its name with tests/test_gpu_detection.py on purpose: tests/conftest.py orders the GPU suite by module
name, and these are kernel-level parity tests."""
import numpy as np
import pytest
import torch

from oracle import assign as A
from oracle import boxes as B
from oracle import nms as N
from oracle import portable_math as PM
from tests import detection_ref as R
from tests import parity_report
from tests.f64_check import bits

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


def cu(a, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.cpu().numpy()


def _in_bound(got, ref, bound, what):
    """|got - ref| <= bound elementwise (where the float64 value is finite) -> the worst error in units of the bound."""
    got = np.asarray(got, f64)
    ok = np.isfinite(ref) & np.isfinite(bound)
    err = np.abs(got - ref)
    bad = ok & ~(err <= bound)
    assert not bad.any(), "%s: %d elements out of bound, first at %s: got %r, float64 %r, bound %r" % (
        what, int(bad.sum()), np.argwhere(bad)[0], got[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])],
        bound[tuple(np.argwhere(bad)[0])])
    live = ok & (bound > 0)
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# ------------------------------------------------------------------------------------------------- anchors
def test_anchors_every_grid_type_count_and_geometry(ops):
    worst = 0.0
    for gh, gw in R.ANCHOR_GRIDS:
        for types, (sc, ar) in R.ANCHOR_TYPES.items():
            for base, stride, offset in R.ANCHOR_GEOMETRY:
                got = host(ops.anchors_generate(gh, gw, sc, ar, base, stride, offset))
                what = "anchors %dx%d, %d types, base %s" % (gh, gw, types, base)
                assert got.shape == (gh * gw * types, 4)
                bits(got, B.grid_anchors(gh, gw, sc, ar, base, stride, offset), what)
                ref, bound = R.anchors64(gh, gw, sc, ar, base, stride, offset)
                worst = max(worst, _in_bound(got, ref, bound, what))
    parity_report.add("detection edges: anchors bit-exact, worst %.2f of the float64 bound" % worst)
    with pytest.raises(Exception, match="1..64"):
        ops.anchors_generate(1, 1, *R.ANCHOR_TOO_MANY)


# ------------------------------------------------------------------------------------------------- prune / clip
@pytest.mark.parametrize("window", R.WINDOWS)
def test_prune_and_clip_at_every_loop_boundary(ops, window):
    for n in R.PRUNE_SIZES:
        b, on, off = R.prune_case(n, window)
        keep = host(ops.prune_outside_window(cu(b), window))
        what = "prune n=%d window %s" % (n, window)
        assert keep.dtype == np.int32 and keep.tolist() == R.prune64(b, window).tolist(), what     # ascending, count exact
        assert keep.tolist() == B.prune_outside_window(b, window)[1].tolist(), what
        assert set(on) <= set(keep.tolist()) and not set(off) & set(keep.tolist()), what
        got = host(ops.clip_to_window(cu(b), window))
        bits(got, B.clip_to_window(b, window, False)[0], "clip n=%d" % n)
        assert (got.astype(f64) == R.clip64(b, window)).all()


# ------------------------------------------------------------------------------------------------- gather / scatter
@pytest.mark.parametrize("batch", R.GATHER_BATCH)
def test_gather_and_scatter_rows(ops, batch):
    for L in R.GATHER_ROW_LEN:
        for n_idx in R.GATHER_N_IDX:
            rng = np.random.RandomState(100 * L + n_idx + batch)
            src = rng.randn(batch, R.GATHER_N_SRC, L).astype(f32)
            idx = rng.permutation(R.GATHER_N_SRC)[:n_idx].astype(np.int32)            # unsorted, unique, in range
            assert n_idx < 2 or (np.diff(idx) < 0).any()
            g = ops.gather_rows(cu(src), cu(idx))
            assert tuple(g.shape) == (batch, n_idx, L)
            bits(host(g), src[:, idx], "gather L=%d n_idx=%d" % (L, n_idx))
            s = host(ops.scatter_rows(g, cu(idx), R.GATHER_N_SRC))
            ref = np.zeros_like(src)
            ref[:, idx] = src[:, idx]
            bits(s, ref, "scatter L=%d n_idx=%d" % (L, n_idx))


# ------------------------------------------------------------------------------------------------- box coder
def test_encode_against_the_fp32_sequence_and_float64(ops):
    worst_u = worst_c = worst_s = 0.0
    for kind in R.CODER_KINDS:
        for n in R.CODER_SIZES:
            b, a = R.coder_case(kind, n)
            for sf in R.SCALE_FACTORS:
                got = host(ops.boxes_encode(cu(b), cu(a), sf))
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    ora = B.encode(b, a, sf)
                what = "encode %s n=%d scale factors %s" % (kind, n, sf)
                print("%s: logf distance %.3f ulps" % (what, R.log_distance(got, b, a, sf)))
                u, c, s = R.check_encode(got, ora, b, a, sf, what)
                worst_u, worst_c, worst_s = max(worst_u, u), max(worst_c, c), max(worst_s, s)
                if kind == "special":
                    assert (got[0] == 0).all(), what                  # a box equal to its anchor: codes of exactly 0
                    if n > 2 and sf[0] == 10.0:
                        assert np.isinf(got[-2, :2]).all(), what
    parity_report.add("detection edges: boxes_encode ty/tx bit-exact, worst %.2f of the float64 bound; th/tw worst %.2f of "
                      "theirs; device logf worst %.3f ulps (LOG_ULPS_MEASURED %.3f, asserted %.3f)"
                      % (worst_c, worst_s, worst_u, R.LOG_ULPS_MEASURED, R.LOG_ULPS))


@pytest.mark.parametrize("batch,batched", [(1, False), (3, False), (3, True), (1, True)])
def test_decode_bit_exact_and_inside_the_float64_bound(ops, batch, batched):
    worst = 0.0
    for kind in R.CODER_KINDS:
        for n in R.CODER_SIZES:
            codes, anc = R.decode_case(kind, batch, n, batched)
            for sf in R.SCALE_FACTORS:
                got = host(ops.boxes_decode(cu(codes), cu(anc), sf))
                for i in range(batch):
                    ai = anc[i] if batched else anc
                    what = "decode %s n=%d image %d scale factors %s" % (kind, n, i, sf)
                    with np.errstate(invalid="ignore", over="ignore"):
                        bits(got[i], B.decode(codes[i], ai, sf), what)
                    ref, bound = R.decode64(codes[i], ai, sf)
                    worst = max(worst, _in_bound(got[i], ref, bound, what))
    parity_report.add("detection edges: boxes_decode (batch %d, per-image anchors %d) bit-exact, worst %.2f of the float64 bound"
                      % (batch, batched, worst))


# ------------------------------------------------------------------------------------------------- target assignment
ALL_OUTPUTS = ("match", "cls_targets", "cls_weights", "reg_targets", "reg_weights")
SUBSETS = (("match",), ("match", "reg_targets"), ("cls_targets", "cls_weights"), ("reg_weights",), ("reg_targets", "cls_weights"))


def _assign(ops, case, mthr, uthr, force, want=ALL_OUTPUTS):
    d = 1 if case["labels"] is None else case["labels"].shape[-1]
    return ops.assign_targets(cu(case["anchors"]), cu(case["gt"]), cu(case["num_gt"]), cu(case["labels"]),
                              cu(R.unmatched_target(d)), mthr, uthr, force, gt_extra=cu(case["extra"]), want=want)


def _oracle_assign(case, b, mthr, uthr, force):
    G = int(case["num_gt"][b])
    d = 1 if case["labels"] is None else case["labels"].shape[-1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return A.assign_targets(R.case_anchors(case, b), case["gt"][b, :G], None if case["labels"] is None else case["labels"][b, :G],
                                R.unmatched_target(d), mthr, uthr, force,
                                gt_closeness=None if case["extra"] is None else case["extra"][b, :G])


def _check_assign_case(ops, case, figures):
    for mthr, uthr in R.THRESHOLDS:
        for force in (False, True):
            out = {k: host(v) for k, v in _assign(ops, case, mthr, uthr, force).items()}
            assert ("extra_targets" in out) == (case["extra"] is not None)
            for b in range(len(case["num_gt"])):
                what = "%s image %d thresholds (%g, %g) force %d" % (case["name"], b, mthr, uthr, force)
                r = _oracle_assign(case, b, mthr, uthr, force)
                assert out["match"][b].tolist() == r["match"].tolist(), what
                figures["left_out"] += R.check_match(out["match"][b], case, b, mthr, uthr, force, what)
                figures["anchors"] += len(r["match"])
                bits(out["cls_targets"][b], r["cls_targets"], what + " cls_targets")
                bits(out["cls_weights"][b], r["cls_weights"], what + " cls_weights")
                bits(out["reg_weights"][b], r["reg_weights"], what + " reg_weights")
                if case["extra"] is not None:
                    bits(out["extra_targets"][b], r["closeness_targets"], what + " extra_targets")
                pos = r["match"] >= 0
                assert (out["reg_targets"][b][~pos].view(np.int32) == 0).all(), what
                G = int(case["num_gt"][b])
                gtb, anc = case["gt"][b, :G][r["match"][pos]], R.case_anchors(case, b)[pos]
                sf = (10.0, 10.0, 5.0, 5.0)
                figures["log"] = max(figures["log"], R.log_distance(out["reg_targets"][b][pos], gtb, anc, sf))
                u, c, s = R.check_encode(out["reg_targets"][b][pos], r["reg_targets"][pos], gtb, anc, sf, what + " reg_targets")
                figures["centre"], figures["size"] = max(figures["centre"], c), max(figures["size"], s)


def _figures():
    return dict(left_out=0, anchors=0, log=0.0, centre=0.0, size=0.0)


def _report_assign(tag, fg):
    parity_report.add("detection edges: assign_targets %s: match / targets / weights bit-exact vs the oracle, %d of %d anchors on a "
                      "knife edge vs float64; reg_targets ty/tx worst %.2f, th/tw worst %.2f of their bounds; device logf worst "
                      "%.3f ulps (LOG_ULPS_MEASURED %.3f)" % (tag, fg["left_out"], fg["anchors"], fg["centre"], fg["size"], fg["log"],
                                                             R.LOG_ULPS_MEASURED))


def test_assign_targets_constructed_edges(ops):
    fg = _figures()
    for case in R.constructed_assign_cases():
        _check_assign_case(ops, case, fg)
    assert fg["left_out"] == 0
    _report_assign("constructed cases", fg)


def test_assign_targets_sizes_batches_and_label_widths(ops):
    fg = _figures()
    for case in R.random_assign_cases():
        _check_assign_case(ops, case, fg)
    _report_assign("random cases", fg)


def test_assign_targets_output_subsets_give_the_same_bits(ops):
    cases = R.assign_cases()
    picks = [c for c in cases if c["name"] in ("duplicate_gt", "anchors_per_image", "tie_grid")] + [c for c in cases if not c["constructed"]][2:5]
    assert len(picks) == 6
    for case in picks:
        for force in (False, True):
            full = _assign(ops, case, 0.7, 0.3, force)
            for want in SUBSETS:
                part = _assign(ops, case, 0.7, 0.3, force, want=want)
                assert set(part) == set(want) | {"match"} | ({"extra_targets"} if case["extra"] is not None else set())
                for k, v in part.items():
                    assert torch.equal(v.view(torch.int32), full[k].view(torch.int32)), (case["name"], want, k)


def test_assign_targets_refuses_more_than_1024_boxes(ops):
    gt = np.zeros((1, 1025, 4), f32)
    with pytest.raises(Exception, match="1..1024"):
        ops.assign_targets(cu(np.zeros((4, 4), f32)), cu(gt), cu(np.array([1], np.int32)), None, cu(np.zeros(1, f32)), 0.7, 0.3, True)


# ------------------------------------------------------------------------------------------------- greedy NMS
def test_greedy_nms_both_algorithms_at_the_edges(ops, monkeypatch):
    knife = total = 0
    for name, bx, sc, max_out, thr, constructed in R.nms_cases():
        ref = N.greedy_nms(bx, sc, max_out, thr)
        got = {}
        for algo in ("greedy", "rounds"):
            monkeypatch.setenv("MTLSSL_NMS_ALGO", algo)
            sel, num = ops.nms(cu(bx), cu(sc), thr, max_out)
            k = int(num.item())
            sel = host(sel)
            assert 0 <= k <= min(max_out, len(bx)) and (sel[k:] == -1).all(), (name, algo)
            got[algo] = sel[:k]
        monkeypatch.delenv("MTLSSL_NMS_ALGO")
        assert got["greedy"].tolist() == got["rounds"].tolist(), name
        assert got["greedy"].tolist() == ref.tolist(), name
        knife += R.check_nms(got["greedy"], bx, sc, max_out, thr, constructed, name)
        total += len(bx)
    bx, sc = R.nms_constructed()
    sel, num = ops.nms(cu(bx), cu(sc), 0.5, 10)
    kept = host(sel)[:int(num.item())].tolist()
    assert 0 in kept and 1 in kept and 2 not in kept and 3 not in kept      # IoU exactly 0.5 suppresses nothing; IoU 1 does
    parity_report.add("detection edges: greedy NMS, both algorithms identical and equal to the oracle on %d cases; %d of %d "
                      "candidates on a knife edge vs float64" % (len(R.nms_cases()), knife, total))
    with pytest.raises(Exception, match="1..4096"):
        ops.nms(cu(bx), cu(sc), 0.5, R.NMS_MAX_OUT_LIMIT + 1)


# ------------------------------------------------------------------------------------------------- multiclass NMS
@pytest.mark.parametrize("algo", ["greedy", "rounds"])
def test_batch_multiclass_nms_at_the_edges(ops, algo, monkeypatch):
    monkeypatch.setenv("MTLSSL_NMS_ALGO", algo)
    worst = 0.0
    for case in R.mc_cases():
        C, c0 = case["C"], case["col0"]
        assert case["scores"].shape[2] == C + c0
        got = ops.batch_multiclass_nms(cu(case["boxes"]), cu(case["scores"]), case["score_thresh"], case["iou"], case["mpc"],
                                       case["max_total"], case["window"], case["frame"], cu(case["num_valid"]), c0, C)
        got = [host(g) for g in got]
        ref = N.batch_multiclass_nms(case["boxes"], case["scores"][:, :, c0:], case["score_thresh"], case["iou"], case["mpc"],
                                     case["max_total"], case["window"], case["num_valid"], case["frame"])
        assert got[3].tolist() == ref[3].tolist(), case["name"]
        bits(got[2], ref[2], case["name"] + " classes")
        bits(got[1], ref[1], case["name"] + " scores")
        if not case["frame"]:
            bits(got[0], ref[0], case["name"] + " boxes")
        worst = max(worst, R.check_mc(got, case, case["name"]))
        for i, k in enumerate(got[3]):                                        # zero padding past the count
            assert not got[0][i, k:].any() and not got[1][i, k:].any() and not got[2][i, k:].any(), case["name"]
    parity_report.add("detection edges: batch multiclass NMS (%s): counts, classes, scores bit-exact on %d cases; boxes in the "
                      "window's frame worst %.2f of 3 roundings" % (algo, len(R.mc_cases()), worst))
    with pytest.raises(Exception, match="1..1024"):
        ops.batch_multiclass_nms(cu(np.zeros((1, 8, 1, 4), f32)), cu(np.zeros((1, 8, 1025), f32)), 0.0, 0.5, 2, 4)


# ------------------------------------------------------------------------------------------------- score converters
@pytest.mark.parametrize("mode", ["SOFTMAX", "SIGMOID"])
def test_score_converters_every_width_and_row_count(ops, mode):
    worst = 0.0
    for C in R.SCORE_C:
        for rows in R.SCORE_ROWS:
            x = R.score_case(rows, C)
            got = host(ops.score_convert(cu(x), mode))
            bits(got, PM.softmax_rn(x) if mode == "SOFTMAX" else PM.sigmoid_rn(x), "%s rows=%d C=%d" % (mode, rows, C))
            d = float(R.ulps32(got, R.softmax64(x) if mode == "SOFTMAX" else R.sigmoid64(x)).max())
            assert d <= 2.0, (mode, rows, C, d)
            worst = max(worst, d)
    parity_report.add("detection edges: score converter %s bit-exact, worst %.2f fp32 ulps of float64 (bound 2)" % (mode, worst))
