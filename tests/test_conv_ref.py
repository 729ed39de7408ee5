"""The yardstick of the float64 plan tests (tests/conv_ref.py) on a CPU: the three references against
torch.nn.functional.conv2d and its autograd in float64 on every row and channel, ConvCase on device "cpu" against a
"kernel" that is the float64 result rounded to float32 — and against mutants of it that its checks must refuse."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mtl_ssl_amd import ops
from tests import conv_ref as R
from tests.parity_report import dot_err

SHAPES = [
    # x shape, filter, stride, dilation, padding
    ((2, 9, 11, 5), (3, 3, 5, 7), 1, 1, "SAME"),
    ((2, 9, 11, 5), (3, 3, 5, 7), 2, 1, "SAME"),
    ((2, 9, 11, 5), (3, 3, 5, 7), 2, 1, "VALID"),
    ((2, 9, 12, 5), (3, 3, 5, 7), 2, 1, "RESNET_SAME"),
    ((1, 10, 8, 4), (3, 3, 4, 6), 1, 2, "SAME"),
    ((2, 7, 7, 6), (1, 1, 6, 5), 1, 1, "SAME"),
    ((1, 12, 13, 3), (7, 7, 3, 8), 2, 1, "SAME"),
]


def _conv64(prob, x, w):
    """The convolution of NHWC x with RSCK w by torch in float64, padded explicitly with the descriptor's pad_t / pad_l
    and the bottom / right pad its output size needs. -> NHWC [N, OH, OW, K], differentiable in x and w."""
    N, H, W, C, K, Rr, S, OH, OW, st, dil, pt, pl = prob
    pb = max((OH - 1) * st + (Rr - 1) * dil + 1 - H - pt, 0)
    pr = max((OW - 1) * st + (S - 1) * dil + 1 - W - pl, 0)
    xp = F.pad(x.double().permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xp, w.double().permute(3, 2, 0, 1), stride=st, dilation=dil)
    return y[:, :, :OH, :OW].permute(0, 2, 3, 1)


def _grads64(prob, x, w, dy):
    x, w = (t.double().clone().requires_grad_() for t in (x, w))
    return torch.autograd.grad((_conv64(prob, x, w) * dy.double()).sum(), (x, w))


@pytest.mark.parametrize("xs,ws,stride,dil,padding", SHAPES, ids=["%s-%dx%d-s%dd%d" % (s[4], s[1][0], s[1][1], s[2], s[3]) for s in SHAPES])
def test_references_match_torch_autograd_in_float64(xs, ws, stride, dil, padding):
    """Every row, every channel. Values of order 1, reductions of at most 147 terms: the worst difference measured over
    all shapes is 3.6e-15; asserted 1e-12."""
    prob = R.prob_of(ops.conv_desc(xs, ws, stride, dil, padding))
    N, H, W, C, K, _, _, OH, OW = prob[:9]
    g = torch.Generator().manual_seed(sum(xs) + stride + dil)
    x, w, dy = (torch.rand(s, generator=g, dtype=torch.float64) - 0.4 for s in (xs, ws, (N, OH, OW, K)))
    dx, dw = _grads64(prob, x, w, dy)
    ch = np.arange
    for what, (ref, mag), want in (
            ("fwd", R._fwd_reference(prob, x, w, ch(N * OH * OW)), _conv64(prob, x, w).reshape(-1, K)),
            ("dgrad", R._dgrad_reference(prob, dy, w, ch(N * H * W)), dx.reshape(-1, C)),
            ("wgrad", R._wgrad_reference(prob, x, dy), dw)):
        assert ref.shape == want.shape and mag.shape == want.shape
        assert float((ref - want).abs().max()) <= 1e-12, what
        assert bool((mag >= ref.abs() - 1e-12).all()), what


def _case():
    """One 3x3 stride-2 problem and, per mode, its float64 results on whole tensors by torch: the linear part and each addend."""
    case = R.ConvCase(R.prob_of(ops.conv_desc((2, 9, 11, 5), (3, 3, 5, 7), 2, 1, "SAME")), device="cpu")
    for mode in (0, 1, 2):
        case.prepare(mode)
    dx, dw = _grads64(case.prob, case.x, case.w, case.dy)
    return case, _conv64(case.prob, case.x, case.w).detach(), dx, dw


def test_conv_case_accepts_the_rounded_float64_result_and_refuses_mutants():
    """|result| <= mag, so rounding it to float32 costs at most one unit: within DIRECT_BOUND. A forgotten residual, a
    forgotten accumulation or a bias gradient without its old value is not."""
    case, y, dx, dw = _case()
    c = case
    bias, res, resd, prev, scale, dw_old, db_old, dy = (t.double() for t in (c.bias, c.res, c.resd, c.prev, c.scale, c.dw_old, c.db_old, c.dy))
    good = {0: (y + bias + res).float(), 1: (dx + resd + prev).float(),
            2: ((dw_old + scale * dw).float(), (db_old + dy.sum((0, 1, 2))).float())}
    for mode, outs in good.items():
        case.check_finite(outs, mode)
        errs = case.check_errors(mode, outs, R.DIRECT_BOUND, "cpu")
        assert len(errs) == (2 if mode == 2 else 1) and max(errs) <= 1.0, (mode, errs)
    mutants = {"residual left out": (0, (y + bias).float()),
               "old value not accumulated": (1, (dx + resd).float()),
               "bias gradient without db_old": (2, (good[2][0], dy.sum((0, 1, 2)).float()))}
    for what, (mode, outs) in mutants.items():
        with pytest.raises(AssertionError):
            case.check_errors(mode, outs, R.DIRECT_BOUND, what)
    with pytest.raises(AssertionError, match="non-finite output"):
        case.check_finite(good[0] * float("nan"))
    # the exact epilogues: relu / where of the linear result pass, one changed bit does not
    case.check_exact_epilogue(0, torch.relu(good[0]), good[0])
    masked = torch.where(c.mask > 0, good[1], torch.zeros_like(good[1]))
    case.check_exact_epilogue(1, masked, good[1])
    with pytest.raises(AssertionError, match="dgrad mask epilogue"):
        case.check_exact_epilogue(1, good[1], good[1])


def test_masked_dgrad_holds_masked_samples_to_zero():
    case, _, dx, _ = _case()
    c = case
    rows = c.sample[1][0]
    sel, ref, mag = R.dgrad_expected(c.prob, c.dy, c.w, rows, resd=c.resd, prev=c.prev, mask=c.mask)
    on = c.mask > 0
    got = torch.where(on, (dx + c.resd.double() + c.prev.double()).float(), torch.zeros(()))
    assert bool((ref[~sel(on)] == 0).all()) and bool((mag[~sel(on)] == 1).all())
    assert dot_err(sel(got), ref, mag) <= 1.0
    r, ch = (~sel(on)).nonzero()[0].tolist()                  # one masked sample of the compared rows
    got.reshape(-1, c.prob[3])[rows[r], ch] = 1e-3
    assert dot_err(sel(got), ref, mag) > R.DIRECT_BOUND


def test_column_subset_is_the_sub_problem():
    """The wide-FC form: expected values on a column subset equal the same columns of the full ones."""
    c = _case()[0]
    for cols, out, expected, args in (
            (np.array([0, 3, 6]), c.res, R.fwd_expected, (c.x, c.w, c.sample[0][0]) + ((c.bias, c.res),)),
            (np.array([1, 4]), c.prev, R.dgrad_expected, (c.dy, c.w, c.sample[1][0]) + ((c.resd, c.prev),))):
        (sel, ref, mag), (sel_s, ref_s, mag_s) = (expected(c.prob, *args[:3], k, *args[3]) for k in (None, cols))
        assert torch.equal(sel_s(out), sel(out)[:, cols])
        assert float((ref_s - ref[:, cols]).abs().max()) <= 1e-12 and float((mag_s - mag[:, cols]).abs().max()) <= 1e-12


def test_small_parts():
    prob = (1, 16, 64, 256, 256, 3, 3, 16, 64, 1, 1, 1, 1)
    assert R.pid(prob) == "1x16x64x256-k256-3x3-o16x64-s1d1p11"
    assert R.pid(prob, 0) == "fwd-1x16x64x256-k256-3x3-o16x64-s1d1p11"
    assert R.pid(prob, 2, "production") == "prod-wgrad-1x16x64x256-k256-3x3"
    assert R.family_lines([("direct", 0, 1.5), ("direct", 0, 0.5), ("direct", 2, 2.0), ("padded", 1, 0.25)]) == [
        "    direct           2 / 0 / 1 cases; worst error in 2^-24*sum|ab| units 1.50 / 0.00 / 2.00",
        "    padded           0 / 1 / 0 cases; worst error in 2^-24*sum|ab| units 0.00 / 0.25 / 0.00"]
    one = np.array([1.0, -0.75, 0.0])
    assert R.fp32_spacing(one).tolist() == [2.0 ** -23, 2.0 ** -24, 2.0 ** -149]      # at 0: the spacing at the smallest normal
    assert R.fp32_ulps(one + 2.0 ** -22, one).tolist()[:2] == [2.0, 4.0]
    tol = R.tanh_tolerance(torch.tensor([2.0], dtype=torch.float64), np.array([0.5]), R.DIRECT_BOUND)
    assert tol.tolist() == [R.DIRECT_BOUND * 2.0 ** -24 * 2.0 + R.TANH_ULPS * 2.0 ** -24]
    assert (R.TANH_ULPS_MEASURED, R.TANH_ULPS) == (1.396, 2.792)
