"""The opt-in split-bf16 fp32 engine (mtl_ssl_amd/csrc/conv_split.h, mtlssl_conv2d_set_fp32_engine): the same
convolutions as the native fp32-MFMA engine, multiplied on the bf16 matrix datapath from operands split exactly
into three bf16 pieces. The claim under test is numerical: against an fp64 reference it is as accurate as the
native engine (both are a few units of 2^-24 * sum|a*b|), on every gather mode it takes over."""
import numpy as np
import pytest
import torch

from tests.parity_report import dot_err as _err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    prev = ops.set_fp32_engine(-1)
    yield ops
    ops.set_fp32_engine(prev)


def _both(ops, fn):
    ops.set_fp32_engine(0)
    a = fn()
    assert ops.set_fp32_engine(1) == 0
    b = fn()
    assert ops.set_fp32_engine(0) == 1
    return a, b


CASES = [
    # (N, H, W, C, K, ksize), forced plan      ROI-tower shapes of config[1] (enough 256x256 tiles for the engine)
    ((600, 7, 7, 512, 2048, 1), 0),
    ((600, 7, 7, 2048, 512, 1), 0),
    ((1300, 7, 7, 256, 256, 3), 0),            # direct 3x3: the nine taps of the implicit GEMM
    ((2, 151, 256, 256, 256, 1), 0),           # a feature-map shaped problem: 77 312 pixels, ragged last row tile
    ((600, 7, 7, 512, 512, 3), 8),             # whole-7-span Winograd: 81 batched GEMMs per pass
    ((40, 28, 40, 256, 256, 3), 4),            # F(4x4,3x3) Winograd: 36 batched GEMMs over 2 800 tiles
    ((16, 38, 64, 512, 512, 3, 1, 2), 0),      # atrous 3x3 (rate 2: R-FCN's block4 on the stride-16 map)
    ((8, 76, 128, 256, 1024, 1, 2, 1), 0),     # stride-2 1x1 (a block's projection shortcut): the strided dgrad gather
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[0])) + "-plan%d" % c[1])
def test_split_engine_is_as_accurate_as_the_native_engine(ops, case):
    (N, H, W, C, K, ks), plan = case[0][:6], case[1]
    stride, dil = (case[0] + (1, 1))[6:8]
    pad = dil * (ks // 2)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.rand(N, H, W, C, device="cuda", generator=g) * 2 - 0.6          # post-ReLU-like: mostly positive
    w = (torch.rand(ks, ks, C, K, device="cuda", generator=g) - 0.5) * (2.0 / np.sqrt(ks * ks * C))
    b = torch.rand(K, device="cuda", generator=g) - 0.5
    d = ops.conv_desc(x.shape, w.shape, stride, dil, "SAME")
    gy = torch.rand(N, d.OH, d.OW, K, device="cuda", generator=g) - 0.5
    try:
        for mode in (0, 1, 2):
            assert ops.force_conv_config(d, mode, plan) == plan      # the big-tile plan the engine replaces
        y0, y1 = _both(ops, lambda: ops.conv2d_fwd(d, x, w, b, None, ops.EPI_BIAS))
        dx0, dx1 = _both(ops, lambda: ops.conv2d_dgrad(d, gy, w))

        def wgrad():
            dw = torch.zeros_like(w)
            ops.conv2d_wgrad(d, x, gy, dw)
            return dw
        dw0, dw1 = _both(ops, wgrad)
        assert not torch.equal(y0, y1) and not torch.equal(dx0, dx1)                 # the other engine ran
        if plan >= 4 or C * K * ks * ks > 9 * 256 * 256:   # too few 256x256 filter tiles to fill the chip: that wgrad stays native
            assert not torch.equal(dw0, dw1)
        # fp64 references: forward / dgrad on a subset of images (the convolution is per image), wgrad on everything
        sub = slice(0, min(N, 6))
        xd, wd, gd = x.double().cpu(), w.double().cpu(), gy.double().cpu()
        xn, gn = xd.permute(0, 3, 1, 2), gd.permute(0, 3, 1, 2)
        wt = wd.permute(3, 2, 0, 1)
        bd = b.double().cpu()
        F = torch.nn.functional
        kw = dict(stride=stride, dilation=dil, padding=pad)
        ref = F.conv2d(xn[sub], wt, bd, **kw).permute(0, 2, 3, 1)
        mag = F.conv2d(xn[sub].abs(), wt.abs(), bd.abs(), **kw).permute(0, 2, 3, 1)
        e0, e1 = _err(y0[sub], ref, mag), _err(y1[sub], ref, mag)
        op = (H - ((d.OH - 1) * stride - 2 * pad + dil * (ks - 1) + 1), W - ((d.OW - 1) * stride - 2 * pad + dil * (ks - 1) + 1))
        refd = F.conv_transpose2d(gn[sub], wt, output_padding=op, **kw).permute(0, 2, 3, 1)
        magd = F.conv_transpose2d(gn[sub].abs(), wt.abs(), output_padding=op, **kw).permute(0, 2, 3, 1)
        f0, f1 = _err(dx0[sub], refd, magd), _err(dx1[sub], refd, magd)
        refw = torch.nn.grad.conv2d_weight(xn, wt.shape, gn, **kw).permute(2, 3, 1, 0)
        magw = torch.nn.grad.conv2d_weight(xn.abs(), wt.shape, gn.abs(), **kw).permute(2, 3, 1, 0)
        g0, g1 = _err(dw0, refw, magw), _err(dw1, refw, magw)
        from tests import parity_report
        parity_report.LINES.append("split-bf16 engine %s plan %d: error in units of 2^-24*sum|ab| — fwd native %.2f split %.2f, "
                                   "dgrad native %.2f split %.2f, wgrad native %.2f split %.2f"
                                   % ("x".join(map(str, case[0])), plan, e0, e1, f0, f1, g0, g1))
        # direct plans sit at the fp32 rounding level on both engines; Winograd adds its transform rounding to both.
        # The split engine is allowed the three dropped products (2 units) on top of what the native engine shows.
        lim = 8 if plan < 4 else 400
        assert e0 < lim and f0 < lim and g0 < lim
        for nat, spl in ((e0, e1), (f0, f1), (g0, g1)):
            assert spl <= 1.25 * max(nat, 1.0) + 2.5
    finally:
        ops.set_fp32_engine(0)
        for mode in (0, 1, 2):
            ops.force_conv_config(d, mode, -1)


def test_small_problems_stay_on_the_native_engine(ops):
    """Fewer than 192 tiles of 256x256: the switch changes nothing, bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(2, 38, 64, 1024, device="cuda", generator=g)
    w = torch.randn(1, 1, 1024, 256, device="cuda", generator=g) / 32
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    y0, y1 = _both(ops, lambda: ops.conv2d_fwd(d, x, w))
    assert torch.equal(y0, y1)


def test_split_engine_on_wide_dynamic_range_and_cancelling_sums(ops):
    """Operands spanning twelve decades with random signs (heavy cancellation inside every dot product), plus exact
    powers of two and values with all 24 mantissa bits set: the split must stay exact where fp32 is exact and lose
    nothing relative to sum|a*b| elsewhere."""
    g = torch.Generator(device="cuda").manual_seed(9)
    N, H, W, C, K = 600, 7, 7, 512, 2048
    mag = 10.0 ** (torch.rand(N, H, W, C, device="cuda", generator=g) * 12 - 6)
    x = mag * (torch.randint(0, 2, mag.shape, device="cuda", generator=g) * 2 - 1)
    x[0, 0, 0, :8] = torch.tensor([1.0, -2.0, 0.5, 16777215.0, -16777215.0, 3.0, 2.0 ** -20, 0.0], device="cuda")
    wm = 10.0 ** (torch.rand(1, 1, C, K, device="cuda", generator=g) * 6 - 3)
    w = wm * (torch.randint(0, 2, wm.shape, device="cuda", generator=g) * 2 - 1)
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    try:
        assert ops.force_conv_config(d, 0, 0) == 0
        y0, y1 = _both(ops, lambda: ops.conv2d_fwd(d, x, w))
        assert bool(torch.isfinite(y1).all())
        xs, ws = x[:4].double().cpu().reshape(-1, C), w.double().cpu().reshape(C, K)
        ref, scale = xs @ ws, xs.abs() @ ws.abs()
        e0 = _err(y0[:4].reshape(-1, K), ref, scale)
        e1 = _err(y1[:4].reshape(-1, K), ref, scale)
        from tests import parity_report
        parity_report.LINES.append("split-bf16 engine, 12 decades of magnitude + random signs: error / (2^-24 sum|ab|) native %.2f split %.2f"
                                   % (e0, e1))
        # with twelve decades inside one sum both engines sit at ~17-20 units (one rounding of the few dominant terms
        # is many units of the small ones); the split engine stays within the same band
        assert e0 < 64 and e1 <= 1.25 * max(e0, 1.0) + 2.5
        # a product of two powers of two is exact on both engines: a one-hot row picks out a single weight
        x2 = torch.zeros(N, H, W, C, device="cuda")
        x2[..., 5] = 2.0 ** -3
        yy0, yy1 = _both(ops, lambda: ops.conv2d_fwd(d, x2, w))
        assert torch.equal(yy0, yy1) and torch.equal(yy1[0, 0, 0], w[0, 0, 5] * 2.0 ** -3)
    finally:
        ops.set_fp32_engine(0)
        ops.force_conv_config(d, 0, -1)
