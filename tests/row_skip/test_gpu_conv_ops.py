"""Row-group activity of the pointwise input / filter gradients (mtlssl_conv2d_dgrad_rs / _wgrad_rs): a call that is
told which RoIs' dy rows are exactly zero leaves them out of its GEMM, and every output bit stays what the unflagged call
computes — launch grids, split boundaries and summation order do not move, and a zero product changes no fp32
accumulator. The yardstick is therefore torch.equal against the same call without flags, for every pointwise tile of
both engines (the whole training step with the switch on against off is in test_gpu_model.py beside this file)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GROUPS, RPG = 11, 49          # 11 RoIs of 7x7 = 539 rows: ragged against the 16-row K-step and every tile height
PATTERNS = {
    "none": [0] * 11,
    "all": [1] * 11,
    "first": [1] + [0] * 10,
    "last": [0] * 10 + [1],
    "alternating": [i & 1 for i in range(11)],
    # groups 2..5 cover rows 98..293: the whole 128-row tile 128..255 (and the 64-row tiles 128..191, 192..255)
    "run_of_four_inactive": [1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1],
}
TILES = [0, 1, 2, 3, 12, 13, 14, 15]     # 128x128, 128x64, 64x64, 256x128 register-staged; the same by LDS-DMA


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope="module")
def operands():
    """Per (C, K): x, w, dy (dense), residual, mask reference, scale — made once, never written."""
    out = {}
    for C, K in ((64, 128), (128, 64)):
        g = torch.Generator().manual_seed(77 + C)
        mk = lambda *s: torch.randn(*s, generator=g).cuda()
        out[(C, K)] = dict(x=mk(GROUPS, 7, 7, C), w=mk(1, 1, C, K) / 8.0, dy=mk(GROUPS, 7, 7, K), res=mk(GROUPS, 7, 7, C),
                           mref=mk(GROUPS, 7, 7, C), scale=torch.rand(K, generator=g).cuda() + 0.5,
                           dw0=mk(1, 1, C, K), db0=mk(K))
    return out


def _masked(dy, flags):
    return (dy * flags.view(-1, 1, 1, 1).to(dy.dtype)).contiguous()


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ck", [(64, 128), (128, 64)])
def test_flagged_gradients_are_bit_identical_to_unflagged(ops, operands, ck, tile):
    C, K = ck
    o = operands[ck]
    d = ops.conv_desc(o["x"].shape, o["w"].shape, 1, 1, "SAME")
    try:
        for mode in (1, 2):
            assert ops.force_conv_config(d, mode, tile) == tile          # the resolver accepts the tile for this shape
        assert ops.conv_plan_info(d, 2)["nsplit"] > 1                    # the filter gradient runs as a multi-split launch
        assert ops.set_row_skip(-1) == 1                                 # on by default
        for name, pat in PATTERNS.items():
            flags = torch.tensor(pat, dtype=torch.uint8, device="cuda")
            dy = _masked(o["dy"], flags)

            def run(active):
                r = [ops.conv2d_dgrad(d, dy, o["w"], active=active),
                     ops.conv2d_dgrad(d, dy, o["w"], o["res"], o["mref"], ops.EPI_RESIDUAL | ops.EPI_MASK, active=active)]
                for beta in (0.0, 1.0):
                    dw, db = o["dw0"].clone(), o["db0"].clone()
                    ops.conv2d_wgrad(d, o["x"], dy, dw, out_scale=o["scale"], dbias=db, beta=beta, active=active)
                    r += [dw, db]
                dw = o["dw0"].clone()
                ops.conv2d_wgrad(d, o["x"], dy, dw, beta=0.0, active=active)          # without dbias: the plain kernels
                return r + [dw]

            ref = run(None)                                              # a null pointer: today's call
            got = run(flags)
            ops.set_row_skip(0)
            off = run(flags)                                             # flags given, switch off
            ops.set_row_skip(1)
            names = ("dgrad", "dgrad+residual+mask", "wgrad beta=0", "dbias beta=0", "wgrad beta=1", "dbias beta=1", "wgrad plain")
            for a, b, c, what in zip(got, ref, off, names):
                assert torch.isfinite(b).all(), (name, what)
                assert torch.equal(a, b), (name, what, "flagged vs unflagged")
                assert torch.equal(c, b), (name, what, "switch off vs unflagged")
            if name == "none":
                assert not got[0].any() and torch.equal(got[2], torch.zeros_like(got[2]))
    finally:
        ops.set_row_skip(1)
        for mode in (1, 2):
            ops.force_conv_config(d, mode, -1)


def test_closeness_tower_shapes_with_their_own_plans(ops):
    """The block4 1x1 layers at 512 RoIs with the plans the table gives them: the 2048 -> 512 input gradient is a main
    launch plus a K-split tail launch, the filter gradients are 8- to 16-way splits on three different tiles. A quarter
    of the RoIs active, scattered."""
    g = torch.Generator().manual_seed(5)
    flags = (torch.rand(512, generator=g) < 0.25).to(torch.uint8).cuda()
    assert 0 < int(flags.sum()) < 512
    gen = torch.Generator(device="cuda").manual_seed(6)
    for C, K in ((512, 2048), (2048, 512)):
        x = torch.randn(512, 7, 7, C, generator=gen, device="cuda")
        w = torch.randn(1, 1, C, K, generator=gen, device="cuda") / 32.0
        dy = _masked(torch.randn(512, 7, 7, K, generator=gen, device="cuda"), flags)
        d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
        out = []
        for active in (None, flags):
            dx = ops.conv2d_dgrad(d, dy, w, None, x, ops.EPI_MASK, active=active)
            dw = torch.zeros_like(w)
            ops.conv2d_wgrad(d, x, dy, dw, beta=0.0, active=active)
            out.append((dx, dw))
        assert torch.equal(out[0][0], out[1][0]), (C, K, "dgrad")
        assert torch.equal(out[0][1], out[1][1]), (C, K, "wgrad")
        assert out[0][1].abs().max() > 0
        del x, w, dy, out
