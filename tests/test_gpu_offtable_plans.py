"""The launch plans off-table image shapes reach, on an MI355X against float64: one case per representative of
tests/golden/offtable_conv_problems.json (tools/offtable_plan_sweep.py: the cheapest problem of every plan signature —
family, plan code, K split, ragged last split, K-split tail launch, ragged tile edges, fold width — that a mixed-aspect
epoch of the shipped configurations reaches and the plan table's own 359 pairs never run; tests/test_offtable_plans.py keeps
the fixture equal to the sweep on a CPU).

Each case first asks the planner (ops.conv_plan_info) and requires the recorded signature, so it cannot pass by running
another plan; then it runs the call the way tests/test_gpu_plan_table.py does (post-ReLU-like x, zero-mean dy, bias,
residual, previous contents for ACCUM, out_scale, dbias with beta = 1) and compares the outputs with the float64
references of tests/conv_ref.py in units of 2^-24 * (sum |a*b| + |addends|): at most 8 for a direct plan, 400 for a Winograd
plan, 8 for the bias gradient. Every output element is compared, with a float64 reference of the whole output built on the
device (ConvCase.check_whole: a miss names row, column, tile and split); before it the sampled reference built on the CPU
runs as before — the independent check of the device's reference, which must equal it on the sample, and the series of
numbers the parity report has carried. The row sample is extended by the places where these plans can go wrong: both sides of the
main / tail boundary and the ends of the tail region, and the last partial Winograd tile along each axis. The ReLU
forward epilogue and the ReLU-mask dgrad epilogue must be exact functions of the linear result, every output finite under
the NaN-poisoned workspaces (conftest: MTLSSL_POISON_WS).

The forward TANH and RELU6 epilogues run once through each of their three sites (in the tile kernel, k_splitk_epilogue
behind a K split with NG % 4 == 0, k_splitk_epilogue_scalar with NG % 4 != 0) on the smallest representatives that reach
them: RELU6 must be clamp(linear, 0, 6) bit for bit; the device tanhf is held to TANH_ULPS (twice the worst distance
measured on an MI355X, see there) from a float64 tanh of the kernel's own fp32 linear output."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import parity_report
from tests.conv_ref import (DIRECT_BOUND, MODE_NAMES, ROWS, TANH_ULPS, TANH_ULPS_MEASURED, WINO_BOUND, ConvCase,  # noqa: F401
                            _rows, family_lines, fp32_ulps, fwd_expected, pid as _pid, plan_test_ops, tanh_tolerance)
from tests.parity_report import dot_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("offtable_plan_sweep", os.path.join(ROOT, "tools", "offtable_plan_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
FIXTURE = json.load(open(TOOL.FIXTURE))
CASES = [(tuple(e["descriptor"]), e["mode"], e["signature"]) for e in FIXTURE["problems"]]
_RUN = {}                       # (problem, mode) -> (family, worst sampled error[, worst whole-output error, elements, reference difference])


@pytest.fixture(scope="module")
def ops():
    yield from plan_test_ops(TOOL.PLANNING_SWITCHES)
    _report()


def _signature(ops, prob, mode):
    return json.loads(json.dumps(TOOL.signature(ops, prob, mode)))


def _boundary_rows(M, info):
    """Flat rows of an M-row GEMM around its K-split tail launch: the first and the last row of the tail region and both
    sides of the main / tail boundary — where launch_planned puts it, (tile rows - tail_rows) * BM, and at
    M - tail_rows * BM (the same row when M is a multiple of BM)."""
    if info["tail_rows"] <= 0:
        return set()
    bm = info["BM"]
    start = (-(-M // bm) - info["tail_rows"]) * bm
    pick = {start, M - 1}
    for b in (start, M - info["tail_rows"] * bm):
        pick.update((b - 1, b, b + 1))
    return {r for r in pick if 0 <= r < M}


def _extra_rows(ops, prob, mode, n_img, hs, ws):
    """Rows (img * hs + y) * ws + x of the compared map (forward output / dgrad input) the plan of this case makes
    interesting, on top of tests/conv_ref.py _rows."""
    d = TOOL.desc_of(prob)
    info = ops.conv_plan_info(d, mode)
    pick = set()
    if info["family"] == "input_parity":
        for c in range(4):
            sub = ops.conv_plan_info(d, mode, c)
            py, px = c >> 1, c & 1
            h2, w2 = (hs - py + 1) // 2, (ws - px + 1) // 2
            for m in _boundary_rows(n_img * h2 * w2, sub):
                n, u, v = m // (h2 * w2), m // w2 % h2, m % w2
                pick.add((n * hs + 2 * u + py) * ws + 2 * v + px)
    elif info["family"].startswith("winograd"):
        t = 4 if info["family"] == "winograd_F43" else 7
        for im in {0, n_img - 1}:
            for y in range(hs // t * t, hs):                     # the last partial tile row
                pick.update((im * hs + y) * ws + x for x in {0, ws // 2, ws - 1})
            for x in range(ws // t * t, ws):                     # the last partial tile column
                pick.update((im * hs + y) * ws + x for y in {0, hs // 2, hs - 1})
    else:
        pick = _boundary_rows(n_img * hs * ws, info)
    return pick


def _sample_rows(ops, prob, mode, n_img, hs, ws, rng):
    extra = _extra_rows(ops, prob, mode, n_img, hs, ws)
    assert len(extra) <= ROWS // 2
    base = _rows(n_img, hs, ws, rng, n=ROWS - len(extra))
    return np.array(sorted(set(base.tolist()) | extra), np.int64)


def test_fixture_is_parametrized_whole():
    assert len(CASES) == FIXTURE["counts"]["representatives"] > 0
    assert len({(p, m) for p, m, _ in CASES}) == len(CASES)
    assert len({json.dumps(s) for _, _, s in CASES}) == len(CASES)      # one representative per signature


@pytest.mark.parametrize("prob,mode,want", CASES, ids=[_pid(p, m) for p, m, _ in CASES])
def test_offtable_plan_matches_float64(ops, prob, mode, want):
    d = TOOL.desc_of(prob)
    case = ConvCase(prob)
    sig = _signature(ops, prob, mode)
    assert sig == want, ("the planner no longer gives this case the plan it stands for", sig, want)
    case.prepare(mode, rows=functools.partial(_sample_rows, ops, prob, mode))
    outs = case.call(ops, d, mode)
    assert _signature(ops, prob, mode) == want, "the plan changed with the first call"
    case.check_finite(outs, MODE_NAMES[mode], sig)

    def note(errs, lims):
        print("%s %s: errors %s of %s (2^-24 * sum|ab| units)" % (_pid(prob, mode), sig[1], ["%.2f" % e for e in errs], lims))
        _RUN[(prob, mode)] = (sig[1], errs[0])
    bound = WINO_BOUND if sig[1].startswith("winograd") else DIRECT_BOUND
    case.check_errors(mode, outs, bound, sig, note)

    def note_whole(errs, lims):
        print("%s %s: every element %s of %s" % (_pid(prob, mode), sig[1], ["%.2f" % e for e in errs], lims))
        st = case.whole_stats[mode]
        _RUN[(prob, mode)] += (errs[0], st["elements"], st["ref_diff"])
    case.check_whole(mode, outs, bound, sig, note_whole)
    if mode < 2:
        case.check_exact_epilogue(mode, case.call(ops, d, mode, nonlinear=True), outs, sig)


def _site(sig):
    """Where the forward epilogue of a direct plan with this signature runs."""
    mode, fam, code, tile, nsplit, ragged, tail, tail_ns, m_bm, ng_bn, ng4 = sig[:11]
    if mode != 0 or fam != "direct" or tail:
        return None                     # (a tail launch folds only its own rows: two sites in one call)
    if nsplit == 1:
        return "in-kernel"
    return "k_splitk_epilogue_scalar" if ng4 else "k_splitk_epilogue"


def test_tanh_and_relu6_epilogues_at_every_site(ops):
    sites = {}
    for prob, mode, sig in sorted(CASES, key=lambda c: TOOL.macs(c[0])):
        s = _site(sig)
        if s is not None:
            sites.setdefault(s, (prob, sig))                            # the smallest representative that reaches the site
    assert set(sites) == {"in-kernel", "k_splitk_epilogue", "k_splitk_epilogue_scalar"}, sorted(sites)
    worst = {}
    for site, (prob, want) in sorted(sites.items()):
        N, H, W, C, K, R, S, OH, OW = prob[:9]
        d = TOOL.desc_of(prob)
        case = ConvCase(prob)
        x, w = case.x, case.w
        assert _signature(ops, prob, 0) == want, (site, want)
        bias = torch.linspace(-8.0, 8.0, K, device="cuda")              # arguments from the linear range to saturation (+-9)
        bias[1:: 4] *= 1.0 / 64.0                                       # ... and a quarter of the channels near 0
        lin = ops.conv2d_fwd(d, x, w, bias, None, ops.EPI_BIAS)
        assert bool(torch.isfinite(lin).all()) and float(lin.min()) < -1.0 and float(lin.max()) > 6.5, site
        # RELU6: exactly clamp(linear, 0, 6)
        y6 = ops.conv2d_fwd(d, x, w, bias, None, ops.EPI_BIAS | ops.EPI_RELU6)
        assert torch.equal(y6, torch.clamp(lin, 0.0, 6.0)), ("RELU6 epilogue", site, want)
        assert bool((y6 == 6.0).any()) and bool((y6 == 0.0).any())
        # TANH: the device tanhf against a float64 tanh of the kernel's own fp32 linear output
        yt = ops.conv2d_fwd(d, x, w, bias, None, ops.EPI_BIAS | ops.EPI_TANH)
        assert bool(torch.isfinite(yt).all())
        lin64 = lin.double().cpu().numpy()
        u = fp32_ulps(yt.double().cpu().numpy(), np.tanh(lin64))
        worst[site] = float(u.max())
        print("tanhf at %s (%s): worst %.3f ulp over %d outputs, arguments %.2f .. %.2f" % (
            site, _pid(prob, 0), worst[site], u.size, lin64.min(), lin64.max()))
        # against float64 end to end: the linear bound plus that term (tanh' <= 1)
        sel, ref, mag = fwd_expected(prob, x, w, _rows(N, OH, OW, case.rng), bias=bias)
        assert dot_err(sel(lin), ref, mag) <= DIRECT_BOUND
        err = np.abs(sel(yt).double().cpu().numpy() - np.tanh(ref.numpy()))
        assert bool((err <= tanh_tolerance(mag, np.tanh(sel(lin).double().cpu().numpy()), DIRECT_BOUND)).all()), site
    parity_report.add("off-table plans, forward TANH epilogue: device tanhf worst %s ulp from float64 tanh of the fp32 "
                      "linear output (asserted: %.2f); RELU6 = clamp(linear, 0, 6) bit for bit at all three sites" % (
                          ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), TANH_ULPS))
    assert max(worst.values()) <= TANH_ULPS, (worst, TANH_ULPS)


def _report():
    if not _RUN:
        return
    parity_report.add("off-table plans (%d representatives of %d signatures reached, %d covered by the plan table); per "
                      "family (fwd / dgrad / wgrad):" % (len(_RUN), FIXTURE["counts"]["signatures_reached"],
                                                         FIXTURE["counts"]["signatures_covered_by_table"]))
    for line in family_lines((fam, mode, *rest) for (prob, mode), (fam, *rest) in _RUN.items()):
        parity_report.add(line)
