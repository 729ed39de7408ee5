"""The yardstick of the float64 plan tests (tests/conv_ref.py) on a CPU: the three sampled references and the three
whole-output ones against torch.nn.functional.conv2d and its autograd in float64 on every row and channel, ConvCase on
device "cpu" against a "kernel" that is the float64 result rounded to float32 — and against mutants of it that its checks
must refuse. The blind-spot mutants are damaged only where the sample is not: the sampled check passes them, the
whole-output check refuses each and names the place."""
import re

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
WHOLE_SHAPES = SHAPES + [
    ((2, 8, 9, 6), (1, 1, 6, 5), 2, 1, "SAME"),             # stride 2, 1x1: input pixels no output reads
    ((1, 11, 10, 4), (3, 3, 4, 6), 1, 2, "VALID"),          # dilation 2
    ((2, 5, 19, 4), (1, 7, 4, 6), 1, 1, "SAME"),            # a 1x7 filter
    ((3, 7, 11, 5), (3, 3, 5, 9), 1, 1, "SAME"),            # OH*OW = 77, M = 231: a multiple of no tile
]
_ids = lambda shapes: ["%s-%dx%d-s%dd%d" % (s[4], s[1][0], s[1][1], s[2], s[3]) for s in shapes]


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


@pytest.mark.parametrize("xs,ws,stride,dil,padding", SHAPES, ids=_ids(SHAPES))
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


def _operands(prob, xs, ws, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(s, generator=g, dtype=torch.float64) - 0.4 for s in (xs, ws, (prob[0], prob[7], prob[8], prob[4]))]


@pytest.mark.parametrize("xs,ws,stride,dil,padding", WHOLE_SHAPES, ids=["%dx%dx%d-%s" % (s[0][0], s[0][1], s[0][2], i) for s, i in zip(WHOLE_SHAPES, _ids(WHOLE_SHAPES))])
def test_whole_references_match_torch_autograd_in_float64(xs, ws, stride, dil, padding, monkeypatch):
    """The whole-output references, every element, in one chunk and in row chunks of a few hundred bytes (whole images
    first, then — one image already too large — row ranges of an image)."""
    prob = R.prob_of(ops.conv_desc(xs, ws, stride, dil, padding))
    N, H, W, C, K, _, _, OH, OW = prob[:9]
    x, w, dy = _operands(prob, xs, ws, sum(xs) + stride + dil)
    dx, dw = _grads64(prob, x, w, dy)
    want = {"fwd": _conv64(prob, x, w).reshape(-1, K), "dgrad": dx.reshape(-1, C), "wgrad": dw, "dbias": dy.sum((0, 1, 2))}
    one_image = 8 * max((H + 8) * (W + 8) * C, OH * OW * max(C, K))     # at least one padded image (pads are below 8)
    for limit, kind in ((R.WHOLE_BYTES, "one"), (one_image, "images"), (3 * OW * max(C, K) * 8, "rows")):
        monkeypatch.setattr(R, "WHOLE_BYTES", limit)
        chunks = R._chunks(prob)
        assert sum((n1 - n0) * (y1 - y0) for n0, n1, y0, y1 in chunks) == N * OH
        if kind == "one":
            assert chunks == [(0, N, 0, OH)]
        elif kind == "images":
            assert all((y0, y1) == (0, OH) for _, _, y0, y1 in chunks)
        else:
            assert all(n1 - n0 == 1 and y1 - y0 <= 3 for n0, n1, y0, y1 in chunks) and len(chunks) >= N * OH // 3
        for what, (ref, mag) in (("fwd", R.fwd_reference_whole(prob, (x, w), "cpu")),
                                 ("dgrad", R.dgrad_reference_whole(prob, (dy, w), "cpu")),
                                 ("wgrad", R.wgrad_reference_whole(prob, (x, dy), "cpu")),
                                 ("dbias", R.dbias_reference_whole(prob, dy, "cpu"))):
            assert ref.shape == want[what].shape and mag.shape == ref.shape and ref.dtype == torch.float64
            assert float((ref - want[what]).abs().max()) <= 1e-12, (what, limit)
            assert bool((mag >= ref.abs() - 1e-12).all()), (what, limit)


def test_stride_2_dgrad_holds_unread_pixels_to_zero():
    """A stride-2 1x1 dgrad: three of four input pixels are read by no output. Their scale is 0 and anything but an exact
    0 there is an infinite error, named by its place — not an exception that hides it."""
    xs, ws = (2, 8, 9, 6), (1, 1, 6, 5)
    prob = R.prob_of(ops.conv_desc(xs, ws, 2, 1, "SAME"))
    N, H, W, C = prob[:4]
    x, w, dy = _operands(prob, xs, ws, 5)
    ref, mag = R.dgrad_reference_whole(prob, (dy, w), "cpu")
    dead = (mag == 0).reshape(N, H, W, C)
    read = torch.zeros(H, W, dtype=torch.bool)
    read[::2, ::2] = True                                               # pad_t = pad_l = 0: the even pixels
    assert prob[11:] == (0, 0) and bool((dead == ~read[None, :, :, None]).all())
    good = ref.float()
    assert R.dot_err_whole(good, ref, mag)[0] <= 1.0
    bad = good.clone()
    at = ((1 * H + 3) * W + 4) * C + 2                                  # image 1, pixel (3, 4): an odd row
    bad.view(-1)[at] = 1e-30
    err, where = R.dot_err_whole(bad, ref, mag)
    assert err == float("inf") and where == at
    assert R.locate(prob, 1, 0, where) == "dx row %d, column 2 (image 1, pixel 3, 4)" % ((1 * H + 3) * W + 4)
    top, beyond = R.worst_whole(bad, ref, mag, R.DIRECT_BOUND)
    assert top[0] == (float("inf"), at) and beyond == 1
    bad.view(-1)[at] = float("nan")
    assert R.dot_err_whole(bad, ref, mag) == (float("inf"), at)
    # through the ReLU mask rule: a masked element is exactly 0 on scale 1
    mask = torch.rand(N, H, W, C, generator=torch.Generator().manual_seed(1)) - 0.5
    ref_m, mag_m = R.dgrad_expected_whole(prob, dy, w, "cpu", mask=mask)
    off = (mask <= 0).reshape(-1, C)
    assert bool((ref_m[off] == 0).all()) and bool((mag_m[off] == 1).all()) and torch.equal(ref_m[~off], ref[~off])


def _blind_case():
    """M = 20 000 rows > 4 * ROWS (the sample is ~1 % of them), C and K beyond 32 and beyond the 16 x 16 channel block."""
    case = R.ConvCase(R.prob_of(ops.conv_desc((2, 100, 100, 40), (3, 3, 40, 36), 1, 1, "SAME")), device="cpu")
    for mode in (0, 1, 2):
        case.prepare(mode)
        case.prepare_whole(mode)
    return case


def _unsampled_run(rows, M, n):
    """First row of the run of n consecutive unsampled rows nearest the middle of M rows — read off the sample."""
    taken = np.zeros(M, bool)
    taken[rows] = True
    free = np.convolve(~taken, np.ones(n, int), "valid") == n          # free[i]: rows i .. i+n-1 are all unsampled
    starts = np.flatnonzero(free)
    assert len(starts), "no run of %d unsampled rows" % n
    r0 = int(starts[np.abs(starts - (M - n) // 2).argmin()])
    assert not set(range(r0, r0 + n)) & set(rows.tolist())
    return r0


def _named(message):
    m = re.search(r"row (\d+), column (\d+)", message)
    assert m, message
    return int(m.group(1)), int(m.group(2))


def test_whole_check_refuses_what_the_sample_cannot_see():
    """The gap and its closure. The "kernel output" is the float64 result rounded to float32; each mutant damages it only
    in places case.sample does not contain (asserted from the sample). check_errors passes all five; check_whole refuses
    each and its message names the damaged row and column."""
    case = _blind_case()
    N, H, W, C, K, Rr, S, OH, OW = case.prob[:9]
    good = {mode: tuple(ref.float() for ref, _ in case.whole[mode]) for mode in (0, 1, 2)}
    for mode in (0, 1, 2):
        outs = good[mode] if mode == 2 else good[mode][0]
        assert max(case.check_errors(mode, outs, R.DIRECT_BOUND, "good")) <= 1.0
        assert max(case.check_whole(mode, outs, R.DIRECT_BOUND, "good")) <= 1.0
        st = case.whole_stats[mode]
        assert st["elements"] == sum(t.numel() for t in good[mode]) and st["ref_diff"] <= 1.0
    assert case.whole_stats[0]["elements"] == N * OH * OW * K and case.whole_stats[2]["elements"] == Rr * S * C * K + K

    def refused(mode, outs, rows_ok, cols_ok, what):
        case.check_errors(mode, outs, R.DIRECT_BOUND, what)              # the sample does not see it
        with pytest.raises(AssertionError) as e:
            case.check_whole(mode, outs, R.DIRECT_BOUND, what)
        row, col = _named(str(e.value))
        assert row in rows_ok and col in cols_ok, (what, row, col, str(e.value)[:300])
        assert what in str(e.value) and "a plain float32 tap walk" in str(e.value)

    for mode in (0, 1):
        M, width = (N * OH * OW, K) if mode == 0 else (N * H * W, C)
        rows, cols = case.sample[mode]
        assert cols is None and M > 4 * R.ROWS and len(rows) == R.ROWS
        r0 = _unsampled_run(rows, M, 32)
        c0 = (width - 32) // 2
        mag = case.whole[mode][0][1]
        # (a) one element of an unsampled row, 64 units of its own scale
        y = good[mode][0].clone()
        y[r0 + 5, 7] += 64 * 2.0 ** -24 * float(mag[r0 + 5, 7])
        refused(mode, y, {r0 + 5}, {7}, "one element")
        # (b) a 32 x 32 patch in the middle of the output zeroed
        y = good[mode][0].clone()
        y[r0:r0 + 32, c0:c0 + 32] = 0
        refused(mode, y, range(r0, r0 + 32), range(c0, c0 + 32), "zeroed patch")
        # (c) two unsampled rows swapped
        y = good[mode][0].clone()
        y[[r0 + 1, r0 + 30]] = y[[r0 + 30, r0 + 1]]
        refused(mode, y, {r0 + 1, r0 + 30}, range(width), "swapped rows")

    cs, ks = case.sample[2]
    c_out, k_out = int(np.setdiff1d(np.arange(C), cs)[3]), int(np.setdiff1d(np.arange(K), ks)[2])
    assert c_out not in cs and k_out not in ks
    dw, db = good[2]
    x64, dy64, scale = case.x.double(), case.dy.double(), case.scale.double()
    # (d) one dw element outside the sampled channel block with one product of its sum left out (tap (1, 1): x itself)
    prod = x64[..., c_out] * dy64[..., k_out]
    n, py, px = np.unravel_index(int(prod.abs().argmax()), prod.shape)
    dw_bad = dw.clone()
    dw_bad[1, 1, c_out, k_out] = float(case.whole[2][0][0][1, 1, c_out, k_out] - scale[k_out] * prod[n, py, px])
    refused(2, (dw_bad, db), {c_out}, {k_out}, "dw product left out")
    # (e) one db column outside the block with one dy left out
    col = dy64[..., k_out]
    db_bad = db.clone()
    db_bad[k_out] = float(case.whole[2][1][0][k_out] - col.reshape(-1)[int(col.abs().argmax())])
    case.check_errors(2, (dw, db_bad), R.DIRECT_BOUND, "db")
    with pytest.raises(AssertionError, match=r"db column %d\b" % k_out):
        case.check_whole(2, (dw, db_bad), R.DIRECT_BOUND, "db")


def test_whole_expected_follows_prepare_and_pins_to_the_sampled_reference():
    """prepare_whole takes the options prepare was given (no residual, the ReLU) and draws nothing; the pin compares on a
    column subset where the sample has one, and refuses a whole reference that is off by more than two summation orders."""
    prob = R.prob_of(ops.conv_desc((2, 9, 11, 5), (3, 3, 5, 7), 2, 1, "SAME"))
    case, twin = (R.ConvCase(prob, device="cpu") for _ in range(2))
    case.prepare(0, cols=lambda width, rng: np.array([0, 3, 6]), res=False, relu=True)
    twin.prepare(0, cols=lambda width, rng: np.array([0, 3, 6]), res=False, relu=True)
    state = case.gen.get_state().clone(), case.rng.bit_generator.state
    (ref, mag), = case.prepare_whole(0)
    assert torch.equal(case.gen.get_state(), state[0]) and case.rng.bit_generator.state == state[1]
    want = torch.relu(_conv64(prob, case.x, case.w).reshape(-1, prob[4]) + case.bias.double())
    assert float((ref - want).abs().max()) <= 1e-12 and bool((ref == 0).any())
    assert case.reference_difference(0) <= 1.0
    rows = case.sample[0][0]
    ref[rows[5], 3] += 1e-9 * float(mag[rows[5], 3])
    with pytest.raises(AssertionError, match="float64 reference on the device against the CPU's"):
        case.reference_difference(0)
    # the next draws are the ones a case without the whole reference makes
    case.prepare(1)
    twin.prepare(1)
    assert torch.equal(case.prev, twin.prev) and np.array_equal(case.sample[1][0], twin.sample[1][0])


def test_locate_names_tile_and_split():
    prob = (2, 100, 100, 40, 36, 3, 3, 100, 100, 1, 1, 1, 1)
    info = dict(family="direct", M=20000, NG=36, BM=128, BN=64, nsplit=2, ks_per_split=5, ksteps=9, tail_rows=3, tail_nsplit=4,
                tail_ks=3, pix_per_split=0)
    assert R.locate(prob, 0, 0, 12345 * 36 + 35, info) == (
        "y row 12345, column 35 (image 1, pixel 23, 45), 128x64 tile (96, 0) of the 20000 x 36 GEMM, K split: 2 splits of 5 of 9 K-steps")
    assert R.locate(prob, 0, 0, 19900 * 36, info).endswith("tile (155, 0) of the 20000 x 36 GEMM, K-split tail launch: 4 splits of 3 K-steps")
    winfo = dict(family="direct", M=40, NG=36, BM=32, BN=32, nsplit=8, pix_per_split=2512)
    assert R.locate(prob, 2, 0, ((1 * 3 + 2) * 40 + 33) * 36 + 34, winfo) == (
        "dw tap (1, 2), row 33, column 34, 32x32 tile (1, 1) of the 40 x 36 GEMM, summed over 8 splits of 2512 pixels")
    assert R.locate(prob, 2, 1, 17, winfo) == "db column 17"
    # an input-parity dgrad: the row of the parity class's own GEMM
    prob2 = (1, 8, 10, 4, 6, 3, 3, 4, 5, 2, 1, 0, 0)
    sub = lambda c: dict(family="input_parity", M=20, NG=4, BM=16, BN=16, nsplit=1, tail_rows=0)
    assert R.locate(prob2, 1, 0, (3 * 10 + 6) * 4 + 1, sub(0), sub) == (
        "dx row 36, column 1 (image 0, pixel 3, 6), parity class 2 row 8, 16x16 tile (0, 0) of the 20 x 4 GEMM")


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
    assert R.family_lines([("direct", 0, 1.5, 5.25, 1000, 0.01), ("direct", 0, 0.5, 3.0, 24, 0.25), ("direct", 2, 2.0, 2.5, 7, 0.125)]) == [
        "    direct           2 / 0 / 1 cases; worst error in 2^-24*sum|ab| units 1.50 / 0.00 / 2.00",
        "        every output element: 1024 / 0 / 7 elements compared; worst error 5.25 / 0.00 / 2.50; float64 reference on the "
        "device against the CPU's on the sample: worst 0.250 of n*2^-52*scale"]
    one = np.array([1.0, -0.75, 0.0])
    assert R.fp32_spacing(one).tolist() == [2.0 ** -23, 2.0 ** -24, 2.0 ** -149]      # at 0: the spacing at the smallest normal
    assert R.fp32_ulps(one + 2.0 ** -22, one).tolist()[:2] == [2.0, 4.0]
    tol = R.tanh_tolerance(torch.tensor([2.0], dtype=torch.float64), np.array([0.5]), R.DIRECT_BOUND)
    assert tol.tolist() == [R.DIRECT_BOUND * 2.0 ** -24 * 2.0 + R.TANH_ULPS * 2.0 ** -24]
    assert (R.TANH_ULPS_MEASURED, R.TANH_ULPS) == (1.396, 2.792)
