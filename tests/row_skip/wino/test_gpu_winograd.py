"""Row-group activity of the 3x3 input / filter gradients on a Winograd plan (mtlssl_conv2d_dgrad_rs / _wgrad_rs with one
flag per batch entry): the active RoIs' tiles are packed to the front of the Winograd planes — whole tiles for the input
gradient, the row pairs one MFMA instruction sums for the filter gradient, inside each split's own range — and the GEMM
stack shrinks with the active share. Packing keeps every accumulator's chain of nonzero terms in its order, so the
yardstick is torch.equal against the same call without flags and against the switch off, as in ../test_gpu_conv_ops.py. The flagged calls of the small problems run on poisoned (NaN) workspaces of exactly the queried size
between guard bands (tests/footprint/guarded.py): a plane row nobody wrote that reached an output would show."""
import pytest
import torch

from tests.footprint.guarded import GuardedWorkspaces

pytestmark = pytest.mark.gpu

GROUPS = 11
PATTERNS = {
    "none": [0] * 11,
    "all": [1] * 11,
    "first": [1] + [0] * 10,
    "last": [0] * 10 + [1],
    "alternating": [i & 1 for i in range(11)],
    "run_of_four_inactive": [1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1],
    # the filter gradient packs pairs of tiles: only second members of a pair / exactly one member of every pair
    "odd_index_only": [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0],
    "one_of_each_pair": [1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 1],
}
# plan codes: 4 * (1 + variant) + tile shape, + 12 for the LDS-DMA engine (ops.force_conv_config)
CODES = {"M7": [8, 9, 10, 11, 20, 21, 22, 23], "F43": [4, 5, 6, 7, 16, 17, 18, 19]}
MAP = {"M7": 7, "F43": 8}              # 7x7: one M7 tile per RoI; 8x8: 2 x 2 F43 tiles per RoI


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


def _operands(n, hw, C, K, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    return dict(x=mk(n, hw, hw, C), w=mk(3, 3, C, K) / 24.0, dy=mk(n, hw, hw, K), res=mk(n, hw, hw, C),
                mref=mk(n, hw, hw, C), scale=torch.rand(K, generator=g).cuda() + 0.5, dw0=mk(3, 3, C, K))


@pytest.fixture(scope="module")
def small():
    """Per (variant, C, K): operands made once, never written."""
    return {(v, C, K): _operands(GROUPS, MAP[v], C, K, 91 + C + MAP[v]) for v in MAP for C, K in ((64, 128), (128, 64))}


def _masked(dy, flags):
    return (dy * flags.view(-1, 1, 1, 1).to(dy.dtype)).contiguous()


def _run(ops, d, o, dy, active, kept=None, wgrad_cases=((0.0, False), (1.0, True))):
    """[dgrad, dgrad + residual + mask] + one filter gradient per (beta, out_scale) case, each without and (if `kept`)
    with the forward's kept input transform."""
    r = [ops.conv2d_dgrad(d, dy, o["w"], active=active),
         ops.conv2d_dgrad(d, dy, o["w"], o["res"], o["mref"], ops.EPI_RESIDUAL | ops.EPI_MASK, active=active)]
    for beta, scaled in wgrad_cases:
        for xf in ((None, kept) if kept is not None else (None,)):
            dw = o["dw0"].clone()
            ops.conv2d_wgrad(d, o["x"], dy, dw, out_scale=o["scale"] if scaled else None, beta=beta, input_xf=xf, active=active)
            r.append(dw)
    return r


def _force(ops, d, code):
    """Pin all three passes of `d` to the Winograd variant of `code` (the forward on the variant's 64x64 tile: it only
    supplies the kept input transform); the resolver must accept the code for this shape."""
    assert ops.force_conv_config(d, 0, code // 4 % 3 * 4 + 2) == code // 4 % 3 * 4 + 2
    for mode in (1, 2):
        assert ops.force_conv_config(d, mode, code) == code


def _unforce(ops, d):
    ops.set_row_skip(1)
    for mode in (0, 1, 2):
        ops.force_conv_config(d, mode, -1)


@pytest.mark.parametrize("ck", [(64, 128), (128, 64)])
@pytest.mark.parametrize("variant,code", [(v, c) for v in ("M7", "F43") for c in CODES[v]])
def test_flagged_winograd_gradients_are_bit_identical_to_unflagged(ops, small, variant, code, ck):
    C, K = ck
    o = small[(variant, C, K)]
    d = ops.conv_desc(o["x"].shape, o["w"].shape, 1, 1, "SAME")
    cases = [(b, s) for b in (0.0, 1.0) for s in (False, True)]
    try:
        _force(ops, d, code)
        assert ops.conv_plan_info(d, 1)["family"] == "winograd_" + variant == ops.conv_plan_info(d, 2)["family"]
        assert ops.set_row_skip(-1) == 1
        keep = {}
        ops.conv2d_fwd(d, o["x"], o["w"], keep_input_xf=keep)
        kept = keep[o["x"].data_ptr()]
        v_before = kept[0].clone()
        for name, pat in PATTERNS.items():
            flags = torch.tensor(pat, dtype=torch.uint8, device="cuda")
            dy = _masked(o["dy"], flags)
            ref = _run(ops, d, o, dy, None, kept, cases)
            with GuardedWorkspaces() as gw:
                got = _run(ops, d, o, dy, flags, kept, cases)
                gw.check()
            ops.set_row_skip(0)
            off = _run(ops, d, o, dy, flags, kept, cases)
            ops.set_row_skip(1)
            for i, (a, b, c) in enumerate(zip(got, ref, off)):
                assert torch.isfinite(b).all(), (name, i)
                assert torch.equal(a, b), (name, i, "flagged vs unflagged")
                assert torch.equal(c, b), (name, i, "switch off vs unflagged")
            if name == "none":
                assert not got[0].any() and not got[2].any()
            else:
                assert got[0].any() and got[2].any()
        assert torch.equal(kept[0], v_before), "the forward's kept transform is an input of the filter gradient"
    finally:
        _unforce(ops, d)


@pytest.mark.parametrize("code", [10, 22, 6, 18])
def test_packing_stays_inside_each_split_of_the_filter_gradient(ops, code):
    """267 RoIs of 7x7, 64 -> 64: the filter gradient's tile range is cut into splits (M7: 267 tiles, F43: 1068), and
    packing must stay inside each split's own range."""
    o = _operands(267, 7, 64, 64, 12)
    d = ops.conv_desc(o["x"].shape, o["w"].shape, 1, 1, "SAME")
    try:
        _force(ops, d, code)
        info = ops.conv_plan_info(d, 2)
        assert info["nsplit"] > 1, info
        tpg = 1 if code // 4 % 3 == 2 else 4                       # tiles per RoI
        assert info["pix_per_split"] % tpg == 0
        edge = info["pix_per_split"] // tpg                        # first RoI of the second split
        assert 8 < edge < 267 - 8
        g = torch.Generator().manual_seed(3)
        pats = {
            "run_across_the_split_boundary": [int(edge - 5 <= i < edge + 6) for i in range(267)],
            "first_split_empty": [int(i >= edge + 3) for i in range(267)],
            "only_first_split": [int(i < edge - 2 and i % 3 == 0) for i in range(267)],
            "quarter_random": (torch.rand(267, generator=g) < 0.25).int().tolist(),
        }
        for name, pat in pats.items():
            flags = torch.tensor(pat, dtype=torch.uint8, device="cuda")
            assert 0 < int(flags.sum()) < 267
            dy = _masked(o["dy"], flags)
            ref = _run(ops, d, o, dy, None)
            with GuardedWorkspaces() as gw:
                got = _run(ops, d, o, dy, flags)
                gw.check()
            for i, (a, b) in enumerate(zip(got, ref)):
                assert torch.isfinite(b).all() and b.any(), (name, i)
                assert torch.equal(a, b), (name, i)
    finally:
        _unforce(ops, d)


def test_closeness_tower_3x3_with_its_own_plans(ops):
    """The closeness tower's 512 -> 512 3x3 layer at 512 RoIs with the plans the table gives it (M7, one tile per RoI), a
    quarter of the RoIs active, scattered — the sampler's cap — and 9 %, the bench's average."""
    gen = torch.Generator(device="cuda").manual_seed(8)
    x = torch.randn(512, 7, 7, 512, generator=gen, device="cuda")
    w = torch.randn(3, 3, 512, 512, generator=gen, device="cuda") / 64.0
    dy_all = torch.randn(512, 7, 7, 512, generator=gen, device="cuda")
    d = ops.conv_desc(x.shape, w.shape, 1, 1, "SAME")
    g = torch.Generator().manual_seed(5)
    for share in (0.25, 0.09):
        flags = (torch.rand(512, generator=g) < share).to(torch.uint8).cuda()
        assert 0 < int(flags.sum()) < 512
        dy = _masked(dy_all, flags)
        out = []
        for active in (None, flags):
            dx = ops.conv2d_dgrad(d, dy, w, None, x, ops.EPI_MASK, active=active)
            dw = torch.zeros_like(w)
            ops.conv2d_wgrad(d, x, dy, dw, beta=0.0, active=active)
            out.append((dx, dw))
        assert ops.conv_plan_info(d, 1)["family"] == "winograd_M7" == ops.conv_plan_info(d, 2)["family"]
        assert torch.equal(out[0][0], out[1][0]), (share, "dgrad")
        assert torch.equal(out[0][1], out[1][1]), (share, "wgrad")
        assert out[0][1].abs().max() > 0 and out[0][0].abs().max() > 0
        del dy, out
