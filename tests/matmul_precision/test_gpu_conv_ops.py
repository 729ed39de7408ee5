"""The float32 matmul precision levels at kernel level (mtl_ssl_amd/csrc/conv_split.h, ops.set_float32_matmul_precision):

  highest  native fp32 MFMA            split   three bf16 pieces per operand, six products (exact split)
  high     two pieces (16 significant bits, truncation), three products
  medium   one bf16 per operand, round-to-nearest-even, one product

What is asserted is derived, not observed: known answers that only the stated product set can give, and the two
inequalities of the accuracy contract against float64, with the native engine's own error measured on the same case:

  high:    |y - y64| <= (3 * 2^-14 + 2^-18) * sum|a||b| + E_native       (3136 units of 2^-24 * sum|a||b|)
  medium:  |y - y64| <= (2^-8 + 2^-18) * sum|a||b| + E_native            (65600 units)

Which engine ran is read from ops.engine_launches, never from bits."""
import numpy as np
import pytest
import torch

from tests import parity_report
from tests.parity_report import dot_err

pytestmark = pytest.mark.gpu

NAMES = ("highest", "split", "high", "medium")
COUNTER = {"highest": "native", "split": "six", "high": "three", "medium": "one"}
# the contract's constants in dot_err's unit, 2^-24 * sum|a||b|
BOUND = {"high": (3 * 2.0 ** -14 + 2.0 ** -18) * 2.0 ** 24, "medium": (2.0 ** -8 + 2.0 ** -18) * 2.0 ** 24}
ONE_BY_ONE = (96, 16, 32, 64, 256)          # 49 152 rows = 192 tiles of 256 x 256: the smallest problem the engine takes


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    prev = ops.get_float32_matmul_precision()
    yield ops
    ops.set_float32_matmul_precision(prev)


def _at(ops, name, fn):
    """fn() under level `name` -> (its result, the launches it made)."""
    ops.set_float32_matmul_precision(name)
    try:
        ops.engine_launches(reset=True)
        out = fn()
        torch.cuda.synchronize()
        return out, ops.engine_launches(reset=True)
    finally:
        ops.set_float32_matmul_precision("highest")


def _only(counts, key, n=None):
    """Launches of one kind only (n of them)."""
    return all(v == 0 for k, v in counts.items() if k != key) and (counts[key] > 0 if n is None else counts[key] == n)


class _Forced:
    """The big-tile plan the engine replaces, pinned for the three passes of one problem."""

    def __init__(self, ops, d, plan):
        self.ops, self.d, self.plan = ops, d, plan

    def __enter__(self):
        for mode in (0, 1, 2):
            assert self.ops.force_conv_config(self.d, mode, self.plan) == self.plan

    def __exit__(self, *exc):
        self.ops.set_float32_matmul_precision("highest")
        for mode in (0, 1, 2):
            self.ops.force_conv_config(self.d, mode, -1)


def _all_bits_weights(shape, gen):
    """Random floats with all 24 significant bits in play: random sign, exponent within 2^-4 .. 2^3, random mantissa."""
    sign = torch.randint(0, 2, shape, device="cuda", generator=gen, dtype=torch.int32) << 31
    expo = torch.randint(123, 131, shape, device="cuda", generator=gen, dtype=torch.int32) << 23
    mant = torch.randint(0, 1 << 23, shape, device="cuda", generator=gen, dtype=torch.int32)
    return (sign | expo | mant).view(torch.float32)


def test_one_hot_rows_show_which_products_ran(ops):
    """x[..., 5] = 1 and 0 elsewhere: every output row is w[0, 0, 5, :] through exactly one product chain, so the result
    IS the operand representation of the level."""
    N, H, W, C, K = ONE_BY_ONE
    gen = torch.Generator(device="cuda").manual_seed(11)
    w = _all_bits_weights((1, 1, C, K), gen)
    # bf16 ties (low half 0x8000) on an even and on an odd bf16, their neighbours, a tie that carries into the exponent,
    # a value whose low byte alone is set, and the same negated
    pats = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x3FFF8000, 0x3FFFFFFF, 0x3F8000FF,
            0x3F80FF00, 0x3F800080, 0x3F800000]
    pats = pats + [p | 0x80000000 for p in pats]
    special = torch.tensor(np.array(pats, dtype=np.uint32).view(np.int32), device="cuda").view(torch.float32)
    w[0, 0, 5, :len(pats)] = special
    x = torch.zeros(N, H, W, C, device="cuda")
    x[..., 5] = 1.0
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    row = w[0, 0, 5]
    want = {"highest": row, "split": row,
            "high": (row.view(torch.int32) & -256).view(torch.float32),          # & 0xFFFFFF00: 16 significant bits
            "medium": row.bfloat16().float()}                                     # round-to-nearest-even
    assert not torch.equal(want["high"], row) and not torch.equal(want["medium"], want["high"])
    assert not torch.equal(want["medium"], (row.view(torch.int32) & -65536).view(torch.float32)), "ties must tell RNE from truncation"
    with _Forced(ops, d, 0):
        for name in NAMES:
            y, counts = _at(ops, name, lambda: ops.conv2d_fwd(d, x, w))
            assert _only(counts, COUNTER[name], None if name == "highest" else 1), (name, counts)
            assert torch.equal(y.reshape(-1, K), want[name].expand(N * H * W, K)), name


def test_integer_exactness_ladder(ops):
    """Integers small enough that every product and partial sum is exact in fp32: `high` (16 significant bits) holds a
    16-bit weight exactly, `medium` computes exactly with the RNE-bf16 weight."""
    N, H, W, C, K = ONE_BY_ONE
    gen = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randint(-8, 9, (N, H, W, C), device="cuda", generator=gen).float()
    w = torch.randint(-2 ** 15, 2 ** 15, (1, 1, C, K), device="cuda", generator=gen).float()
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    # |sum| <= 64 * 8 * 2^15 = 2^24: float64 holds these integers exactly, so this IS the int64 result
    exact = lambda wt: (x.reshape(-1, C).double() @ wt.reshape(C, K).double()).long()
    with _Forced(ops, d, 0):
        yh, ch = _at(ops, "high", lambda: ops.conv2d_fwd(d, x, w))
        ym, cm = _at(ops, "medium", lambda: ops.conv2d_fwd(d, x, w))
    assert _only(ch, "three", 1) and _only(cm, "one", 1), (ch, cm)
    assert torch.equal(yh.reshape(-1, K).double().long(), exact(w)) and torch.equal(yh, yh.round())
    assert torch.equal(ym.reshape(-1, K).double().long(), exact(w.bfloat16().float())) and torch.equal(ym, ym.round())
    assert not torch.equal(ym, yh)


def _inputs(shape, ks, seed=3):
    """As tests/test_gpu_split_engine.py: mostly-positive activations, zero-mean weights."""
    N, H, W, C, K = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(N, H, W, C, device="cuda", generator=g) * 2 - 0.6
    w = (torch.rand(ks, ks, C, K, device="cuda", generator=g) - 0.5) * (2.0 / np.sqrt(ks * ks * C))
    gy = torch.rand(N, H, W, K, device="cuda", generator=g) - 0.5
    return x, w, gy


def _check_bounds(ops, tag, fn, ref, mag, sub=slice(None), launches=1):
    """The contract's two inequalities for one pass of one case; E_native from the `highest` run of the same case."""
    y0, c0 = _at(ops, "highest", fn)
    assert _only(c0, "native"), (tag, c0)
    e_native = dot_err(y0[sub], ref, mag)
    seen = {"highest": e_native}
    for name in ("high", "medium"):
        y, c = _at(ops, name, fn)
        assert _only(c, COUNTER[name], launches), (tag, name, c)          # the reduced kernel ran, and nothing else
        seen[name] = dot_err(y[sub], ref, mag)
    line = "matmul precision %s: error / (2^-24 sum|a||b|) — highest %.2f, high %.1f (bound %.0f + highest), medium %.1f (bound %.0f + highest)" % (
        tag, e_native, seen["high"], BOUND["high"], seen["medium"], BOUND["medium"])
    parity_report.LINES.append(line)
    print(line)
    assert e_native < 8                      # the native engine sits at the fp32 rounding level (test_gpu_split_engine.py)
    for name in ("high", "medium"):
        assert seen[name] <= BOUND[name] + e_native, (tag, name, seen)
    return seen


@pytest.mark.parametrize("shape", [(96, 16, 32, 64, 512), (97, 16, 31, 64, 512)], ids=["192x2-tiles", "ragged-rows"])
def test_forward_1x1_bounds(ops, shape):
    N, H, W, C, K = shape
    assert (N * H * W) % 256 == (0 if shape[0] == 96 else 240)
    x, w, _ = _inputs(shape, 1)
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    xs, ws = x.reshape(-1, C).double(), w.reshape(C, K).double()
    ref, mag = (xs @ ws).cpu().reshape(N, H, W, K), (xs.abs() @ ws.abs()).cpu().reshape(N, H, W, K)
    with _Forced(ops, d, 0):
        _check_bounds(ops, "fwd 1x1 %s" % "x".join(map(str, shape)), lambda: ops.conv2d_fwd(d, x, w), ref, mag)


def test_dgrad_1x1_bounds(ops):
    shape = N, H, W, C, K = (96, 16, 32, 256, 64)
    _, w, gy = _inputs(shape, 1)
    d = ops.conv_desc((N, H, W, C), w.shape, 1, 1, "SAME")
    gs, wt = gy.reshape(-1, K).double(), w.reshape(C, K).double().t()
    ref, mag = (gs @ wt).cpu().reshape(N, H, W, C), (gs.abs() @ wt.abs()).cpu().reshape(N, H, W, C)
    with _Forced(ops, d, 0):
        _check_bounds(ops, "dgrad 1x1 %s" % "x".join(map(str, shape)), lambda: ops.conv2d_dgrad(d, gy, w), ref, mag)


def test_direct_3x3_bounds(ops):
    """The nine taps of the implicit GEMM (the general gather instantiation), forward and data gradient; float64 on the
    first 6 images (the convolution is per image)."""
    shape = N, H, W, C, K = (1300, 7, 7, 256, 256)
    x, w, gy = _inputs(shape, 3)
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    sub = slice(0, 6)
    F = torch.nn.functional
    xn, gn = x[sub].double().cpu().permute(0, 3, 1, 2), gy[sub].double().cpu().permute(0, 3, 1, 2)
    wt = w.double().cpu().permute(3, 2, 0, 1)
    ref = F.conv2d(xn, wt, padding=1).permute(0, 2, 3, 1)
    mag = F.conv2d(xn.abs(), wt.abs(), padding=1).permute(0, 2, 3, 1)
    refd = F.conv_transpose2d(gn, wt, padding=1).permute(0, 2, 3, 1)
    magd = F.conv_transpose2d(gn.abs(), wt.abs(), padding=1).permute(0, 2, 3, 1)
    with _Forced(ops, d, 0):
        _check_bounds(ops, "fwd 3x3 1300x7x7x256x256", lambda: ops.conv2d_fwd(d, x, w), ref, mag, sub)
        _check_bounds(ops, "dgrad 3x3 1300x7x7x256x256", lambda: ops.conv2d_dgrad(d, gy, w), refd, magd, sub)


def test_filter_gradient_bounds(ops):
    """16 384 pixels, 4 filter tiles x 64 pixel cuts: the smallest shape the engine's filter-gradient plan accepts."""
    shape = N, H, W, C, K = (8, 32, 64, 512, 512)
    x, w, gy = _inputs(shape, 1)
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    xs, gs = x.reshape(-1, C).double(), gy.reshape(-1, K).double()
    ref, mag = (xs.t() @ gs).cpu().reshape(1, 1, C, K), (xs.abs().t() @ gs.abs()).cpu().reshape(1, 1, C, K)

    def wgrad():
        dw = torch.zeros_like(w)
        ops.conv2d_wgrad(d, x, gy, dw)
        return dw
    with _Forced(ops, d, 0):
        _check_bounds(ops, "wgrad 1x1 8x32x64x512x512", wgrad, ref, mag)


def test_winograd_gemms_stay_six_product(ops):
    """The Winograd transforms amplify operand error a hundredfold, so no reduced product set runs there: under `high` and
    `medium` the whole-7-span plan computes what it computes under `split`, bit for bit, with six-product launches only."""
    shape = (600, 7, 7, 512, 512)
    x, w, gy = _inputs(shape, 3)
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")

    def wgrad():
        dw = torch.zeros_like(w)
        ops.conv2d_wgrad(d, x, gy, dw)
        return dw
    with _Forced(ops, d, 8):
        for fn in (lambda: ops.conv2d_fwd(d, x, w), lambda: ops.conv2d_dgrad(d, gy, w), wgrad):
            y1, c1 = _at(ops, "split", fn)
            assert _only(c1, "six"), c1
            for name in ("high", "medium"):
                y, c = _at(ops, name, fn)
                assert c == c1, (name, c, c1)
                assert torch.equal(y, y1), name


def test_small_problems_stay_on_the_native_engine(ops):
    """Fewer than 192 tiles of 256 x 256: no level changes anything, bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(2, 38, 64, 1024, device="cuda", generator=g)
    w = torch.randn(1, 1, 1024, 256, device="cuda", generator=g) / 32
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    y0, c0 = _at(ops, "highest", lambda: ops.conv2d_fwd(d, x, w))
    assert _only(c0, "native"), c0
    for name in NAMES[1:]:
        y, c = _at(ops, name, lambda: ops.conv2d_fwd(d, x, w))
        assert c == c0 and torch.equal(y, y0), (name, c)


@pytest.mark.parametrize("name", NAMES)
def test_rerun_is_bit_identical(ops, name):
    shape = (96, 16, 32, 64, 512)
    x, w, _ = _inputs(shape, 1, seed=8)
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    with _Forced(ops, d, 0):
        a, ca = _at(ops, name, lambda: ops.conv2d_fwd(d, x, w))
        b, cb = _at(ops, name, lambda: ops.conv2d_fwd(d, x, w))
    assert _only(ca, COUNTER[name], None if name == "highest" else 1) and ca == cb
    assert torch.equal(a, b)
