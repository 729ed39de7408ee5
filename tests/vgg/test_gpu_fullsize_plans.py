"""Every convolution the Faster R-CNN VGG-16 configuration launches, at the size production runs it, on an MI355X against
float64: one case per entry of tests/golden/vgg16_conv_problems.json (tools/vgg16_plan_sweep.py; tests/vgg/test_host_plans.py
keeps the fixture equal to the sweep on a CPU) — the `production` list, every (problem, mode) of one training step of
configs/vgg16/frcnn_vgg16_voc_mtl.config at 600x1024 and batch 1 under freeze_layer 'conv2' and '', and the
`representatives`, the cheapest problem of every plan signature other frames or batch 2 reach and nothing else shows.

Each case first asks the planner (ops.conv_plan_info) and requires the recorded signature, so it cannot pass by running
another plan; then it makes the call the way tests/test_gpu_plan_table.py does (post-ReLU-like x, zero-mean dy, forward
with bias and residual, dgrad with residual accumulated into previous contents, wgrad with out_scale, dbias and beta = 1)
and compares the outputs with the float64 references of tests/conv_ref.py in units of 2^-24 * (sum |a*b| + |addends|):
at most 8 for a direct, padded, thin or valu_fallback plan, 400 for a Winograd plan, 8 for the bias gradient. Every output
element is compared, all 4096 columns of the wide FC layers included, with a float64 reference of the whole output built on
the device (ConvCase.check_whole: a miss names row, column, tile and split). Before it the sampled reference built on the
CPU runs as before: it is the independent check of the device's reference, which must equal it on the sample, and keeps the
parity report's series. Neither shortens a reduction. Rows of the sample: tests/conv_ref.py _rows plus the K-split tail boundaries and the last
partial Winograd tile (tests/test_gpu_offtable_plans.py _extra_rows); the FC problems have at most 640 rows and every one is
compared. Where C = 25 088 or K = 4096 the CPU reference is built on a sample of at least 64 output columns, tile boundaries
included (a float64 copy of the 25 088 x 4096 filter is 822 MB); the filter gradient is sampled by channel blocks as for
every other layer. After conv1_1's forward — the VALU fallback indexed per element, on the largest map of the project — the
whole last row and last column of the frame and its corners are compared as well. The ReLU forward epilogue and the
ReLU-mask dgrad epilogue must be exact functions of the linear result, a second call must give the same bits, and every
output must be finite under the NaN-poisoned workspaces (conftest: MTLSSL_POISON_WS).

test_one_step_launches_the_production_list builds the full configuration, runs one Trainer.forward_backward at 600x1024 and
requires that the (mode, problem) set the step launched is the fixture's production list for freeze_layer 'conv2': the host
enumeration cannot miss a launch without this suite noticing."""
import functools
import importlib.util
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import parity_report
from tests.conv_ref import (DIRECT_BOUND, MODE_NAMES, ROWS, WINO_BOUND, ConvCase, _channels, _rows, family_lines, fwd_expected,
                            dgrad_expected, pid, plan_test_ops)
from tests.parity_report import dot_err
from tests.test_gpu_offtable_plans import _extra_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COLS = 64                       # sampled output columns of the wide FC layers
# The FC reductions of this configuration are the longest in the project: 25 088 terms, 392 K-steps folded from up to 8
# splits (the plan table's longest is a few thousand terms). Measured on an MI355X, in 2^-24 * sum|ab| units, worst over
# the compared outputs (every row, 64 columns), kernel / a torch CPU float32 matmul of the same operands on the same outputs:
#   25 088 -> 4096 forward   64 rows (K split 8)  0.76 / 0.23      264 rows (K split 4, partial tile)  1.30 / 0.34
#   25 088 -> 4096 dgrad     64 rows (K split 3, ragged)  1.12 / 0.35      128 rows                     1.04 / 0.38
#    4096 -> 4096  forward   64 rows (K split 8)  0.66 / 0.41      264 rows (K split 4, partial tile)  1.11 / 0.43
#    4096 -> 4096  dgrad     64 rows (K split 8)  0.67 / 0.37
# The kernel is well inside DIRECT_BOUND (the zero-mean filter keeps the partial sums far below sum|ab|), so these cases are
# held to it like every other direct plan; each run prints both figures again and the parity report carries them.
FC_BOUND = DIRECT_BOUND


def _tool():
    spec = importlib.util.spec_from_file_location("vgg16_plan_sweep", os.path.join(ROOT, "tools", "vgg16_plan_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
FIXTURE = json.load(open(TOOL.FIXTURE))
CASES = [(name, tuple(e["descriptor"]), e["mode"], e["signature"])
         for name in ("production", "representatives") for e in FIXTURE[name]]
_RUN = {}                       # (list, problem, mode) -> (family, worst sampled error[, worst whole-output error, elements, reference difference])
_FC = {}                        # (problem, mode) -> (kernel error, torch CPU float32 error) of the long FC reductions
_T0 = [None]


def _pid(name, prob, mode):
    return pid(prob, mode, name)


@pytest.fixture(scope="module")
def ops():
    for o in plan_test_ops(TOOL.PLANNING_SWITCHES):
        _T0[0] = time.time()
        yield o
    torch.cuda.empty_cache()
    _report()


def _signature(ops, prob, mode):
    return json.loads(json.dumps(TOOL.signature(ops, prob, mode)))


def _is_fc(prob):
    return prob[1:3] == (1, 1) and prob[5:9] == (1, 1, 1, 1)


def _wide_fc(prob):
    """The layers whose float64 filter does not fit a few seconds: FC_0_4096 (25 088 -> 4096) and FC_1_4096 (4096 -> 4096)."""
    return _is_fc(prob) and (prob[3] == 25088 or prob[4] == 4096)


def _sample_rows(ops, prob, mode, n_img, hs, ws, rng):
    if _is_fc(prob):
        assert n_img <= 640
        return np.arange(n_img)                                         # every row of an FC problem
    extra = _extra_rows(ops, prob, mode, n_img, hs, ws)
    assert len(extra) <= ROWS // 2
    base = _rows(n_img, hs, ws, rng, n=ROWS - len(extra))
    return np.array(sorted(set(base.tolist()) | extra), np.int64)


def _columns(prob, width, rng):
    """Output columns the reference is built on: all of them, or for the wide FC layers COLS of them — the 64 / 128 /
    256 tile boundaries, the last column, the rest at random."""
    if not _wide_fc(prob) or width <= COLS:
        return np.arange(width)
    cols = _channels(width, rng, n=COLS)
    assert len(cols) >= COLS and {0, 63, 64, 127, 128, 255, 256, width - 1} <= set(cols.tolist())
    return cols


def _frame_edge_rows(OH, OW):
    """conv1_1: three corners of the frame and its whole last row and last column (the fourth corner is on both)."""
    pick = {0, OW - 1, (OH - 1) * OW}
    pick.update((OH - 1) * OW + x for x in range(OW))
    pick.update(y * OW + OW - 1 for y in range(OH))
    return np.array(sorted(pick), np.int64)


def test_fixture_is_parametrized_whole():
    c = FIXTURE["counts"]
    assert len(CASES) == c["production"] + c["representatives"] and c["production"] > 0 and c["representatives"] > 0
    assert len({(p, m) for _, p, m, _ in CASES}) == len(CASES)
    reps = [json.dumps(s) for name, _, _, s in CASES if name == "representatives"]
    assert len(set(reps)) == len(reps)                                  # one representative per signature
    assert not set(reps) & {json.dumps(s) for name, _, _, s in CASES if name == "production"}


@pytest.mark.parametrize("name,prob,mode,want", CASES, ids=[_pid(n, p, m) for n, p, m, _ in CASES])
def test_vgg16_plan_matches_float64(ops, name, prob, mode, want):
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    d = TOOL.desc_of(prob)
    case = ConvCase(prob)
    x, w, dy = case.x, case.w, case.dy
    sig = _signature(ops, prob, mode)
    assert sig == want, ("the planner no longer gives this case the plan it stands for", sig, want)
    case.prepare(mode, rows=functools.partial(_sample_rows, ops, prob, mode), cols=functools.partial(_columns, prob))
    call = functools.partial(case.call, ops, d, mode)
    outs = call()
    cpu32 = None
    if _wide_fc(prob) and mode < 2:                                     # the same outputs by a torch CPU float32 matmul
        rows, cols = case.sample[mode]
        rows_t, cols_t = torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()
        if mode == 0:
            mm, (_, ref, mag) = x.reshape(N, C)[rows_t].cpu() @ w[..., cols_t].reshape(C, -1).cpu(), fwd_expected(prob, x, w, rows, cols)
        else:
            mm, (_, ref, mag) = dy.reshape(N, K)[rows_t].cpu() @ w.reshape(C, K)[cols_t].t().cpu(), dgrad_expected(prob, dy, w, rows, cols)
        cpu32 = dot_err(mm, ref, mag)
    if mode == 0 and C == 3:                                            # conv1_1: the frame's border, element by element
        edge = _frame_edge_rows(OH, OW)
        sel, ref, mag = fwd_expected(prob, x, w, edge, case.sample[0][1], case.bias, case.res)
        e_edge = dot_err(sel(outs), ref, mag)
        print("%s: last row, last column and corners of the frame (%d pixels): %.2f" % (_pid(name, prob, mode), len(edge), e_edge))
        assert e_edge <= DIRECT_BOUND, ("conv1_1 frame border", e_edge)

    assert _signature(ops, prob, mode) == want, "the plan changed with the first call"
    case.check_finite(outs, MODE_NAMES[mode], sig)

    def note(errs, lims):
        print("%s %s: errors %s of %s (2^-24 * sum|ab| units)%s" % (
            _pid(name, prob, mode), sig[1], ["%.2f" % e for e in errs], lims,
            "" if cpu32 is None else "; torch CPU float32 on the same outputs %.2f" % cpu32))
        _RUN[(name, prob, mode)] = (sig[1], errs[0])
        if cpu32 is not None:
            _FC[(prob, mode)] = (errs[0], cpu32)
    wino = sig[1].startswith("winograd")
    bound = WINO_BOUND if wino else (FC_BOUND if _wide_fc(prob) else DIRECT_BOUND)
    case.check_errors(mode, outs, bound, sig, note)

    def note_whole(errs, lims):                                         # every column, also where `cols` restricts the sample
        print("%s %s: every element %s of %s" % (_pid(name, prob, mode), sig[1], ["%.2f" % e for e in errs], lims))
        st = case.whole_stats[mode]
        _RUN[(name, prob, mode)] += (errs[0], st["elements"], st["ref_diff"])
    case.check_whole(mode, outs, bound, sig, note_whole)
    case.whole.clear()

    # a second call gives the same bits (the K-split fold and the Winograd transforms sum in a fixed order)
    again = call()
    for a, b in zip(again if mode == 2 else (again,), outs if mode == 2 else (outs,)):
        assert torch.equal(a, b), ("two calls differ", MODE_NAMES[mode], sig)
    del again
    if mode < 2:
        case.check_exact_epilogue(mode, call(nonlinear=True), outs, sig)


def test_one_step_launches_the_production_list(ops):
    """One Trainer.forward_backward of the full configuration at 600x1024, batch 1, plan table on, tuner off: the keys of
    ops._tuned — every (mode, problem) the step launched — are the fixture's production pairs for freeze_layer 'conv2'."""
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    want = {(e["mode"],) + tuple(e["descriptor"]) for e in FIXTURE["production"] if "conv2" in e["freeze_layers"]}
    assert len(want) > 40
    cfg = config.parse_pipeline_config(open(TOOL.CONFIG).read())
    assert str(cfg.model.faster_rcnn.feature_extractor.freeze_layer) == "conv2"
    dev = torch.device("cuda", 0)
    t0 = time.time()
    # what a step launches does not depend on the weights: the six 25 088 x 4096 / 4096 x 4096 matrices (18 s of host
    # truncated-normal draws) are tiled from one 2^20-element block of the same distribution; everything else initialises
    # as in production
    block = (np.random.default_rng(0).standard_normal(1 << 20).clip(-2, 2) * 0.01).astype(np.float32)
    values = {s.name: np.resize(block, s.shape) for s in model_builder.variable_specs(cfg.model, True) if s.size >= 1 << 24}
    assert len(values) == 6, sorted(values)
    model = model_builder.build(cfg.model, True, dev, seed=0, values=values)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    torch.cuda.synchronize()
    t_build = time.time() - t0
    batch = synthetic.make_batch(1, 600, 1024, int(cfg.model.faster_rcnn.num_classes), seed=1234, device=dev)
    ops.reset_tuning(use_plan_db=True, autotune=False)
    try:
        t0 = time.time()
        losses = tr.forward_backward(batch)
        torch.cuda.synchronize()
        t_step = time.time() - t0
        launched = set(ops._tuned)
        model.check_device_flags()
        assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    finally:
        ops.reset_tuning(use_plan_db=True, autotune=False)
        del tr, model, batch
        torch.cuda.empty_cache()
    line = ("vgg16 full configuration: one step at 600x1024 launched %d (mode, problem) pairs, the host enumeration lists %d; "
            "model build %.2f s, first forward_backward %.2f s" % (len(launched), len(want), t_build, t_step))
    print(line)
    parity_report.add(line)
    assert launched == want, ("launched, not enumerated", sorted(launched - want), "enumerated, not launched", sorted(want - launched))


def _report():
    if not _RUN:
        return
    c = FIXTURE["counts"]
    parity_report.add("vgg16 plans at full size (%d production pairs, %d representatives; %d signatures reached, %d covered by the "
                      "plan table or the off-table fixture); per family (fwd / dgrad / wgrad):" % (
                          sum(1 for k in _RUN if k[0] == "production"), sum(1 for k in _RUN if k[0] == "representatives"),
                          c["signatures_reached"], c["signatures_covered_by_table_or_offtable"]))
    for line in family_lines((fam, mode, *rest) for (name, prob, mode), (fam, *rest) in _RUN.items()):
        parity_report.add(line)
    for (prob, mode), (e, e32) in sorted(_FC.items()):
        parity_report.add("    FC %d rows, %d -> %d, %s (%d-term reduction): kernel %.2f, torch CPU float32 matmul on the same "
                          "outputs %.2f (asserted: %.0f)" % (prob[0], prob[3], prob[4], MODE_NAMES[mode],
                                                             prob[4] if mode == 1 else prob[3], e, e32, FC_BOUND))
    parity_report.add("    wall time of tests/vgg/test_gpu_fullsize_plans.py: %.0f s" % (time.time() - _T0[0]))
