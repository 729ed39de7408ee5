"""CPU checks of tests/detection_ref.py, the float64 definitions and case tables of the detection-kernel edge tests
(tests/detection_edges/test_gpu_detection.py): the definitions give the reference's own answers (the golden vectors),
the fp32 oracle agrees with them on every case table off the knife edges and inside the caps, every constructed case
hits the edge it is named after, and every wrong variant (`mutate=`) is told apart by at least one case."""
import json
import os

import numpy as np
import pytest

from oracle import assign as A
from oracle import boxes as B
from oracle import nms as N
from oracle import portable_math as PM
from tests import detection_ref as R

f32, f64 = np.float32, np.float64
# numpy's vectorised float32 log, which oracle/boxes.py encode() uses, is documented to 3.83 ulps (numpy
# core/src/umath/loops_exponent_log.dispatch.c.src); the scale product adds less than one. The device's logf is held to
# LOG_ULPS by the GPU module, not here.
NUMPY_LOG_ULPS = 5.0


@pytest.fixture(scope="module")
def vec(golden_dir):
    with open(os.path.join(golden_dir, "reference_vectors.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def npg(golden_dir):
    return np.load(os.path.join(golden_dir, "np_box_golden.npz"))


# ------------------------------------------------------------------------------------- the reference's own answers
def test_coder_definitions_give_the_golden_codes(vec):
    v = vec["coder"]
    one = (1.0, 1.0, 1.0, 1.0)
    np.testing.assert_allclose(R.encode64(v["boxes"], v["anchors"], one), v["codes_noscale"], rtol=1e-5, atol=1e-6)   # the vectors hold 6 decimals
    np.testing.assert_allclose(R.encode64(v["boxes"], v["anchors"], v["scale_factors"]), v["codes_scaled"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(R.decode64(v["codes_noscale"], v["anchors"], one)[0], v["boxes"], rtol=1e-6, atol=1e-5)
    np.testing.assert_allclose(R.decode64(v["codes_scaled"], v["anchors"], v["scale_factors"])[0], v["boxes"], rtol=1e-6, atol=1e-5)
    # the graph is fp32: the box 10 .. 10.0000001 has height 0 there, and the EPSILON alone keeps the logarithm finite
    np.testing.assert_allclose(R.encode64(np.array(v["tiny_box"], f32), np.array(v["tiny_anchor"], f32), one), v["tiny_codes"],
                               rtol=1e-5, atol=1e-6)


def test_anchor_definition_gives_the_golden_anchors(vec):
    for key in ("anchors_single", "anchors_grid"):
        v = vec[key]
        a, bound = R.anchors64(v["grid"][0], v["grid"][1], v["scales"], v["aspect_ratios"], v["base"], v["stride"], v["offset"])
        np.testing.assert_allclose(a, v["expected"], rtol=1e-6, atol=1e-5)
        assert (bound <= 4 * R.EPS * np.abs(a).max()).all()


def test_box_definitions_give_the_golden_answers(vec, npg):
    v = vec["box_ops"]
    np.testing.assert_allclose(R.iou64(v["c1"], v["c2"]), v["iou"], rtol=1e-6)
    np.testing.assert_allclose(R.clip64(v["clip_in"], v["window"]), v["clip_unfiltered"])
    assert R.prune64(v["prune_in"], v["window"]).tolist() == v["prune_keep"]
    np.testing.assert_allclose(R.change_frame64(v["frame_in"], v["frame_window"]), v["frame_out"], rtol=1e-6)
    b1, b2 = npg["b1"], npg["b2"]
    np.testing.assert_allclose(R.iou64(b1, b2), npg["iou"], rtol=2e-6, atol=1e-7)
    c = R.clip64(b2, npg["window"])
    c = c[(c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1]) > 0]
    np.testing.assert_allclose(c, npg["clip"], rtol=1e-6)
    assert R.prune64(b2, npg["window"]).tolist() == npg["prune_idx"].tolist()
    np.testing.assert_allclose(R.change_frame64(b2, npg["window"]), npg["change_frame"], rtol=1e-5, atol=1e-6)


def test_nms_definitions_give_the_golden_selections(vec, npg):
    v = vec["nms_clusters"]
    bx = np.array(v["boxes"], f32)
    for c in v["cases"]:
        sel, _, _ = R.greedy_nms64(bx, v["scores"], c["max"], v["iou_thresh"])
        np.testing.assert_allclose(bx[sel], c["expected"])
    i = v["identical"]
    sel, _, _ = R.greedy_nms64([i["box"]] * i["n"], [i["score"]] * i["n"], i["max"], v["iou_thresh"])
    assert sel.tolist() == [0]
    nb, sc = npg["nms_boxes"], npg["nms_scores"]
    for thr in (0.3, 0.5, 0.7):
        sel, _, _ = R.greedy_nms64(nb, sc, 100, thr)
        np.testing.assert_allclose(nb[sel], npg["nms_out_%d" % int(thr * 10)])
        np.testing.assert_allclose(sc[sel], npg["nms_out_scores_%d" % int(thr * 10)])


def test_multiclass_definition_gives_the_golden_detections(vec):
    for m in vec["multiclass_nms_cases"]:
        n_exp = len(m["exp_scores"])
        T = m["max_total"] or 16
        ob, os_, oc, on, _ = R.batch_multiclass_nms64(np.array(m["boxes"], f32)[None], np.array(m["scores"], f32)[None],
                                                      m["score_thresh"], m["iou_thresh"], m["max_per_class"], T,
                                                      m["clip_window"], m["change_frame"])
        assert on[0] == n_exp, m["name"]
        np.testing.assert_allclose(ob[0, :n_exp], m["exp_corners"], rtol=1e-6, err_msg=m["name"])
        np.testing.assert_allclose(os_[0, :n_exp], m["exp_scores"], rtol=1e-6, err_msg=m["name"])
        np.testing.assert_allclose(oc[0, :n_exp], m["exp_classes"], err_msg=m["name"])
    for m in vec["batch_multiclass_nms_cases"]:
        ob, os_, oc, on, _ = R.batch_multiclass_nms64(np.array(m["boxes"], f32), np.array(m["scores"], f32), m["score_thresh"],
                                                      m["iou_thresh"], m["max_per_class"], m["max_total"])
        np.testing.assert_allclose(ob, m["exp_corners"], rtol=1e-6, err_msg=m["name"])
        np.testing.assert_allclose(os_, m["exp_scores"], rtol=1e-6, err_msg=m["name"])
        np.testing.assert_allclose(oc, m["exp_classes"], err_msg=m["name"])
        np.testing.assert_array_equal(on, m["exp_num"])


def test_matcher_definition_gives_the_golden_matches(vec):
    for c in vec["matcher"]:
        if not c["nlu"] or c["matched"] is None:
            continue
        ut = c["matched"] if c["unmatched"] is None else c["unmatched"]
        assert R.match64(np.array(c["sim"], f64), c["matched"], ut, c["force"]).tolist() == c["expected"], c


# ------------------------------------------------------------------------------------- the fp32 oracle on the tables
def test_oracle_anchors_prune_clip_agree_with_float64():
    for gh, gw in R.ANCHOR_GRIDS:
        for sc, ar in R.ANCHOR_TYPES.values():
            for base, stride, offset in R.ANCHOR_GEOMETRY:
                ref, bound = R.anchors64(gh, gw, sc, ar, base, stride, offset)
                got = B.grid_anchors(gh, gw, sc, ar, base, stride, offset)
                assert got.shape == ref.shape and (np.abs(got - ref) <= bound).all()
    assert len(R.ANCHOR_TOO_MANY[0]) * len(R.ANCHOR_TOO_MANY[1]) == 65
    for n in R.PRUNE_SIZES:
        for win in R.WINDOWS:
            b, on, off = R.prune_case(n, win)
            keep = B.prune_outside_window(b, win)[1]
            assert keep.tolist() == R.prune64(b, win).tolist()
            assert set(on) <= set(keep.tolist()) and not set(off) & set(keep.tolist())
            assert len(on) == len(off) == min(4, n // 2)
            np.testing.assert_array_equal(B.clip_to_window(b, win, False)[0].astype(f64), R.clip64(b, win))
            if n > 20:
                assert 0 < len(keep) < n


def test_oracle_coder_agrees_with_float64():
    worst = 0.0
    for kind in R.CODER_KINDS:
        for n in R.CODER_SIZES:
            b, a = R.coder_case(kind, n)
            for sf in R.SCALE_FACTORS:
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    ora = B.encode(b, a, sf)
                u, _, _ = R.check_encode(ora, ora, b, a, sf, "oracle encode %s n=%d %s" % (kind, n, sf), NUMPY_LOG_ULPS)
                worst = max(worst, u)
                if kind == "special":
                    assert (ora[0] == 0).all()                        # a box equal to its anchor: codes of exactly 0
                    if n > 1:
                        assert not np.isfinite(R.encode64(b, a, sf)[-1]).all() or np.abs(ora[-1]).max() > 1e6
                for batch, batched in ((1, False), (3, False), (3, True)):
                    codes, anc = R.decode_case(kind, batch, n, batched)
                    for i in range(batch):
                        ai = anc[i] if batched else anc
                        ref, bound = R.decode64(codes[i], ai, sf)
                        with np.errstate(invalid="ignore", over="ignore"):
                            got = B.decode(codes[i], ai, sf)
                        assert (np.abs(got - ref) <= bound).all(), (kind, n, sf, batch, batched)
    assert worst <= NUMPY_LOG_ULPS


def _oracle_assign(case, b, mthr, uthr, force):
    G = int(case["num_gt"][b])
    d = 1 if case["labels"] is None else case["labels"].shape[-1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return A.assign_targets(R.case_anchors(case, b), case["gt"][b, :G], None if case["labels"] is None else case["labels"][b, :G],
                                R.unmatched_target(d), mthr, uthr, force,
                                gt_closeness=None if case["extra"] is None else case["extra"][b, :G])


def test_oracle_assignment_agrees_with_float64_inside_the_caps():
    left_out = 0
    for case in R.assign_cases():
        for mthr, uthr in R.THRESHOLDS:
            for force in (False, True):
                for b in range(len(case["num_gt"])):
                    r = _oracle_assign(case, b, mthr, uthr, force)
                    what = "%s image %d thresholds (%g, %g) force %d" % (case["name"], b, mthr, uthr, force)
                    left_out += R.check_match(r["match"], case, b, mthr, uthr, force, what)
                    pos = r["match"] >= 0
                    G = int(case["num_gt"][b])
                    R.check_encode(r["reg_targets"][pos], r["reg_targets"][pos], case["gt"][b, :G][r["match"][pos]],
                                   R.case_anchors(case, b)[pos], (10.0, 10.0, 5.0, 5.0), what, NUMPY_LOG_ULPS)
    assert left_out <= 8                                   # a handful over the whole table; each case is capped inside


def test_oracle_nms_agrees_with_float64_inside_the_caps():
    for name, bx, sc, max_out, thr, constructed in R.nms_cases():
        R.check_nms(N.greedy_nms(bx, sc, max_out, thr), bx, sc, max_out, thr, constructed, name)
    for case in R.mc_cases():
        C, c0 = case["C"], case["col0"]
        got = N.batch_multiclass_nms(case["boxes"], case["scores"][:, :, c0:c0 + C], case["score_thresh"], case["iou"], case["mpc"],
                                     case["max_total"], case["window"], case["num_valid"], case["frame"])
        R.check_mc(got, case, case["name"])


def test_oracle_score_converters_agree_with_float64():
    for C in R.SCORE_C:
        for rows in R.SCORE_ROWS:
            x = R.score_case(rows, C)
            assert float(R.ulps32(PM.softmax_rn(x), R.softmax64(x)).max()) <= 2.0
            assert float(R.ulps32(PM.sigmoid_rn(x), R.sigmoid64(x)).max()) <= 2.0


# ------------------------------------------------------------------------------------- every constructed case hits its edge
def test_constructed_assignment_cases_hit_their_edges():
    kinds = set()
    for case in R.constructed_assign_cases():
        e = case["edge"]
        kinds.add(e["kind"])
        a0 = R.case_anchors(case, 0)
        G = int(case["num_gt"][0])
        s64 = R.iou64(case["gt"][0, :G], a0)
        s32 = B.iou(case["gt"][0, :G], a0)
        assert (s32.astype(f64) == s64).all(), case["name"]          # every IoU of a constructed case is exact in fp32
        if e["kind"] == "threshold":
            for col, t in e["on"].items():
                assert s32[col, col] == f32(t) and s64[col, col] == t
                assert 0 < s64[col + 1, col + 1] - t < R.KNIFE and 0 < t - s64[col + 2, col + 2] < R.KNIFE
            assert {0.75, 0.5, 0.25} <= {t for pair in R.THRESHOLDS for t in pair}
        elif e["kind"] == "row_tie":
            p, q = e["cols"]
            row = s64[e["row"]]
            assert row[p] == row[q] == row.max() == 0.5 and (row == row.max()).sum() == 2
            want = {"tie_wave": lambda: p // 64 == q // 64,
                    "tie_block": lambda: p // 64 != q // 64 and p // 256 == q // 256,
                    "tie_grid": lambda: p // 256 != q // 256,
                    "tie_grid_last_block": lambda: p // 256 == 0 and q // 256 == (len(a0) - 1) // 256 == 2}[case["name"]]
            assert want(), case["name"]
        elif e["kind"] == "same_column":
            cols = s64.argmax(1)
            assert len(e["rows"]) >= 2 and all(cols[r] == e["col"] for r in e["rows"])
            assert R.match64(s64, 0.7, 0.3, True)[e["col"]] == max(e["rows"])
        elif e["kind"] == "zero_row":
            for r in e["rows"]:
                assert (s64[r] == 0).all()
            assert R.match64(s64, 0.7, 0.3, True)[0] == max(list(e["rows"]) + ([e["also"]] if "also" in e else []))
            if "also" in e:
                assert s64[e["also"]].argmax() == 0 and s64[e["also"], 0] > 0
        elif e["kind"] == "batched":
            assert case["anchors"].ndim == 3 and not (case["anchors"][0] == case["anchors"][1]).all()
            assert 0 in case["num_gt"].tolist()
    assert kinds == {"threshold", "row_tie", "same_column", "zero_row", "batched"}
    # the padding rows of every case are NaN: a kernel that read one would show it
    for case in R.assign_cases():
        for b, g in enumerate(case["num_gt"]):
            assert np.isnan(case["gt"][b, g:]).all()


def test_constructed_nms_cases_hit_their_edges():
    bx, sc = R.nms_constructed()
    q, valid = R._nms_iou64(bx[0].astype(f64), bx.astype(f64))
    assert q[1] == 0.5 and q[2] == 1.0 and q[3] == 1.0 and not valid[4] and not valid[7]
    assert R._nms_iou64(bx[5].astype(f64), bx[6:7].astype(f64))[0][0] == 0.75
    assert R._nms_iou64(bx[8].astype(f64), bx[9:10].astype(f64))[0][0] == 1.0 / 3.0
    sel = R.greedy_nms64(bx, sc, 10, 0.5)[0].tolist()
    assert 0 in sel and 1 in sel and 2 not in sel                    # IoU == threshold: neither box of the pair goes
    assert R.greedy_nms64(bx, sc, 10, 1.0)[0].tolist() == np.argsort(-sc, kind="stable").tolist()
    assert N._nms_iou_gt(bx[0], bx[1], 0.5) is False and N._nms_iou_gt(bx[0], bx[1], np.nextafter(f32(0.5), f32(0))) is True
    # the cross-class tie: equal scores survive in all three classes and max_total cuts inside the group
    case = R.mc_cross_class_tie()
    ob, os_, oc, on, sure = R.batch_multiclass_nms64(case["boxes"], case["scores"], case["score_thresh"], case["iou"], case["mpc"], 16)
    assert on[0] == 7 and sorted(set(oc[0, 1:7].tolist())) == [0.0, 1.0, 2.0] and (os_[0, 1:7] == 0.5).all()
    assert 1 < case["max_total"] < 7
    ob, os_, oc, on, sure = R.batch_multiclass_nms64(case["boxes"], case["scores"], case["score_thresh"], case["iou"], case["mpc"],
                                                     case["max_total"])
    assert oc[0].tolist() == [1.0, 0.0, 0.0, 1.0] and ob[0, 3].tolist() == [0, 0, 10, 10]
    assert (case["scores"] == case["score_thresh"]).any()
    # the table: scores on the threshold everywhere, a cut inside a tie group, max_total beyond C * mpc, mpc beyond n
    cut = beyond = over_n = False
    for case in R.mc_cases():
        C, c0 = case["C"], case["col0"]
        s = case["scores"][:, :, c0:c0 + C]
        if case["name"] not in ("one_box", "iou_on_threshold"):
            assert (s == case["score_thresh"]).any(), case["name"]
        args = (case["boxes"], s, case["score_thresh"], case["iou"], case["mpc"])
        rest = (case["window"], case["frame"], case["num_valid"])
        T = case["max_total"]
        full = R.batch_multiclass_nms64(*args, T + 8, *rest)
        for i in range(len(full[3])):
            if full[3][i] > T and full[1][i, T - 1] == full[1][i, T] and full[2][i, T - 1] != full[2][i, T]:
                cut = True
        beyond |= T > C * min(case["mpc"], s.shape[1])
        over_n |= case["mpc"] > s.shape[1]
    assert cut and beyond and over_n


# ------------------------------------------------------------------------------------- the cases discriminate
@pytest.mark.parametrize("mutant", R.MATCH_MUTANTS)
def test_every_matcher_mutant_is_caught(mutant):
    caught = []
    for case in R.assign_cases():
        for mthr, uthr in R.THRESHOLDS:
            for force in (False, True):
                for b in range(len(case["num_gt"])):
                    G = int(case["num_gt"][b])
                    sim = R.iou64(case["gt"][b, :G], R.case_anchors(case, b))
                    if (R.match64(sim, mthr, uthr, force, mutant) != R.match64(sim, mthr, uthr, force)).any():
                        caught.append(case["name"])
    assert set(caught) & {c["name"] for c in R.constructed_assign_cases()}, caught      # by a constructed case, not by luck


def test_the_nms_and_merge_mutants_are_caught():
    hit = [name for name, bx, sc, max_out, thr, _ in R.nms_cases()
           if R.greedy_nms64(bx, sc, max_out, thr, "iou_ge")[0].tolist() != R.greedy_nms64(bx, sc, max_out, thr)[0].tolist()]
    assert any(h.startswith("constructed") for h in hit), hit
    for mutant in ("score_ge", "iou_ge") + R.MERGE_MUTANTS:
        hit = []
        for case in R.mc_cases():
            C, c0 = case["C"], case["col0"]
            args = (case["boxes"], case["scores"][:, :, c0:c0 + C], case["score_thresh"], case["iou"], case["mpc"], case["max_total"],
                    case["window"], case["frame"], case["num_valid"])
            a, b = R.batch_multiclass_nms64(*args), R.batch_multiclass_nms64(*args, mutate=mutant)
            if any((x != y).any() for x, y in zip(a[:4], b[:4])):
                hit.append(case["name"])
        assert hit, mutant
        if mutant in R.MERGE_MUTANTS:
            assert "cross_class_tie" in hit, (mutant, hit)


def test_the_coder_mutant_is_caught():
    hit = 0
    for kind in R.CODER_KINDS:
        for n in R.CODER_SIZES:
            b, a = R.coder_case(kind, n)
            for sf in R.SCALE_FACTORS:
                with np.errstate(divide="ignore", invalid="ignore"):
                    ref, mut = R.encode64(b, a, sf), R.encode64(b, a, sf, mutate="no_epsilon")
                ok = np.isfinite(ref).all(1)
                cb = R.encode_center_bound(b, a, sf)
                hit += int((~np.isfinite(mut[ok])).any() or (np.abs(mut[ok, :2] - ref[ok, :2]) > cb[ok]).any())
    assert hit
