"""Footprint of the convolution family: every plan family and engine mode runs with its workspace, its inputs and its
outputs between guard bands (tests/footprint/guarded.py), each exactly as large as the size query or the tensor shape
says. Asserted per case: every guard intact, the NaN-prefilled output finite everywhere (full coverage),
conv_plan_info reports the family the case stands for, and sampled rows stay within the suite's existing float64
bounds (tests/conv_ref.py: DIRECT_BOUND / WINO_BOUND units of 2^-24 * sum|a*b|; Winograd also within the 1e-4 of
tests/test_gpu_winograd.py; the split engine and the precision levels within the bounds of
tests/test_gpu_split_engine.py and tests/matmul_precision). No buffer is ever smaller than its query says."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from tests import parity_report
from tests.conv_ref import (DIRECT_BOUND, WINO_BOUND, _channels, _rows, dgrad_expected, fwd_expected, prob_of as _prob,
                            tanh_tolerance, wgrad_expected)
from tests.footprint.guarded import GuardedOutputs, GuardedWorkspaces, GuardSet, check_guards
from tests.parity_report import dot_err
from tests.test_gpu_conv_ops import NULL_WS_CASES

pytestmark = pytest.mark.gpu

TILES = [0, 1, 2, 3, 12, 13, 14, 15]     # 128x128, 128x64, 64x64, 256x128 register-staged; the same by LDS-DMA
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


def _lib():
    from mtl_ssl_amd.lib import lib
    return lib()


def _err(got, ref, mag):
    """dot_err; an output whose every scale is 0 (all-zero operands) must be exactly 0 everywhere."""
    if not bool((mag > 0).any()):
        assert not bool(got.any())
        return 0.0
    return dot_err(got, ref, mag)


def _relerr(got, ref):
    return float((got.double().cpu() - ref).abs().max() / (ref.abs().max() + 1e-30))


class Run:
    """One problem: its operands (as tests/test_gpu_conv_ops.py draws them for the float64 plan tests) held once as
    guarded inputs, every call under GuardedWorkspaces with guarded outputs, every result checked on sampled rows."""

    def __init__(self, ops, d, seed, tag):
        self.ops, self.d, self.tag = ops, d, tag
        N, H, W, C, K, R, S, OH, OW = d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.OH, d.OW
        g = torch.Generator(device="cuda").manual_seed(seed)
        rand = lambda *s: torch.rand(*s, device="cuda", generator=g)
        self.o = dict(x=rand(N, H, W, C) * 2 - 0.6, w=(rand(R, S, C, K) - 0.5) * (2.0 / np.sqrt(R * S * C)),
                      dy=rand(N, OH, OW, K) - 0.5, bias=rand(K) - 0.5, res=rand(N, OH, OW, K) - 0.5,
                      resd=rand(N, H, W, C) - 0.5, mref=rand(N, H, W, C) - 0.5, scale=rand(K) + 0.5,
                      dw_old=rand(R, S, C, K) - 0.5, db_old=rand(K) - 0.5, dx_old=rand(N, H, W, C) - 0.5)
        self.rng = np.random.default_rng(seed)
        self.gs = GuardSet()
        self.g = {k: self.gs.input(v, k) for k, v in self.o.items() if k not in ("dw_old", "db_old", "dx_old")}
        self.ws = {}                     # (what) -> workspace bytes handed out

    def set_dy(self, dy):
        self.o["dy"] = dy
        self.g["dy"] = self.gs.input(dy, "dy")

    def _done(self, gw, what, outs):
        gw.check()
        self.gs.check()
        for name, t in outs:
            assert bool(torch.isfinite(t).all()), (self.tag, what, name, "not written everywhere (NaN prefill left)")
        self.ws[what] = sum(n for _, n, _ in gw.handouts)

    # ---- forward
    def fwd(self, epi_names=("BIAS", "RESIDUAL"), bound=DIRECT_BOUND, d=None, out=None, **kw):
        ops, d0, o, g = self.ops, self.d, self.o, self.g
        d = d or d0
        epi = sum(getattr(ops, "EPI_" + e) for e in epi_names)
        y = out if out is not None else self.gs.output((d0.N, d0.OH, d0.OW, d0.K), "y")
        with GuardedWorkspaces() as gw:
            ops.conv2d_fwd(d, g["x"], g["w"], g["bias"] if "BIAS" in epi_names else None,
                           g["res"] if "RESIDUAL" in epi_names else None, epi, out=y, **kw)
        self._done(gw, "fwd", [("y", y)])
        sel, ref, mag = fwd_expected(_prob(d0), o["x"], o["w"], _rows(d0.N, d0.OH, d0.OW, self.rng),
                                     bias=o["bias"] if "BIAS" in epi_names else None,
                                     res=o["res"] if "RESIDUAL" in epi_names else None, relu="RELU" in epi_names)
        got = sel(y)
        if "TANH" in epi_names:
            t64 = torch.tanh(ref)
            err = (got.double().cpu() - t64).abs()
            worst = float((err / torch.from_numpy(tanh_tolerance(mag, t64, bound))).max())
            assert worst <= 1.0, (self.tag, "fwd tanh", worst)
            return y
        e = dot_err(got, ref, mag)
        print("%s fwd: error %.2f of %.0f (2^-24 * sum|ab| units), workspace %d B" % (self.tag, e, bound, self.ws["fwd"]))
        assert e <= bound, (self.tag, "fwd", e)
        if bound == WINO_BOUND:
            assert _relerr(got, ref) < 1e-4, (self.tag, "fwd")
        self.err = e
        return y

    # ---- data gradient
    def dgrad(self, bound=DIRECT_BOUND, d=None, dy=None, active=None, epi_names=("RESIDUAL", "MASK"), **kw):
        ops, d0, o, g = self.ops, self.d, self.o, self.g
        d = d or d0
        epi = sum(getattr(ops, "EPI_" + e) for e in epi_names)
        accum = "ACCUM" in epi_names                 # accumulates into old values; otherwise a NaN prefill proves full coverage
        dx = self.gs.output(None, "dx", fill=o["dx_old"]) if accum else self.gs.output((d0.N, d0.H, d0.W, d0.C), "dx")
        with GuardedWorkspaces() as gw:
            ops.conv2d_dgrad(d, dy if dy is not None else g["dy"], g["w"], g["resd"] if "RESIDUAL" in epi_names else None,
                             g["mref"] if "MASK" in epi_names else None, epi, out=dx, active=active, **kw)
        self._done(gw, "dgrad", [("dx", dx)])
        sel, ref, mag = dgrad_expected(_prob(d0), o["dy"], o["w"], _rows(d0.N, d0.H, d0.W, self.rng),
                                       resd=o["resd"] if "RESIDUAL" in epi_names else None, prev=o["dx_old"] if accum else None,
                                       mask=o["mref"] if "MASK" in epi_names else None)
        got = sel(dx)
        if "MASK" in epi_names:
            assert bool((got.cpu()[~(sel(o["mref"]) > 0).cpu()] == 0).all()), (self.tag, "masked gradient must be exactly 0")
        if float(mag.max()) == 0.0:                  # no active row at all: every output is exactly 0
            assert not bool(dx.any()), (self.tag, "dgrad of all-zero dy")
            return dx
        e = dot_err(got, ref, mag)
        print("%s dgrad: error %.2f of %.0f (2^-24 * sum|ab| units), workspace %d B" % (self.tag, e, bound, self.ws["dgrad"]))
        assert e <= bound, (self.tag, "dgrad", e)
        if bound == WINO_BOUND:
            assert _relerr(got, ref) < 1e-4, (self.tag, "dgrad")
        self.err = e
        return dx

    # ---- filter gradient (+ per-channel scale, bias gradient; beta 0 overwrites a NaN prefill, beta 1 accumulates)
    def wgrad(self, beta, bound=DIRECT_BOUND, d=None, dy=None, active=None, input_xf=None):
        ops, d0, o, g = self.ops, self.d, self.o, self.g
        d = d or d0
        if beta:
            dw = self.gs.output(None, "dw", fill=o["dw_old"])
            db = self.gs.output(None, "dbias", fill=o["db_old"])
        else:
            dw = self.gs.output((d0.R, d0.S, d0.C, d0.K), "dw")
            db = self.gs.output((d0.K,), "dbias")
        with GuardedWorkspaces() as gw:
            ops.conv2d_wgrad(d, g["x"], dy if dy is not None else g["dy"], dw, out_scale=g["scale"], dbias=db, beta=beta,
                             active=active, input_xf=input_xf)
        self._done(gw, "wgrad", [("dw", dw), ("dbias", db)])
        assert gw.bytes_of("wgrad") == [_lib().conv2d_wgrad_workspace_bytes(ctypes.byref(d))]
        cs, ks = _channels(d0.C, self.rng), _channels(d0.K, self.rng)
        pairs = [(sel(t), ref, mag) for t, (sel, ref, mag) in zip((dw, db), wgrad_expected(
            _prob(d0), o["x"], o["dy"], cs, ks, o["scale"], beta, o["dw_old"], o["db_old"]))]
        errs = [_err(*p) for p in pairs]
        print("%s wgrad beta %g: errors %s of %.0f / %.0f, workspace %d B" % (self.tag, beta, ["%.2f" % e for e in errs], bound,
                                                                               DIRECT_BOUND, self.ws["wgrad"]))
        assert errs[0] <= bound and errs[1] <= DIRECT_BOUND, (self.tag, "wgrad", errs)      # dbias: a plain column sum
        if bound == WINO_BOUND:
            assert _relerr(*pairs[0][:2]) < 1e-4, (self.tag, "wgrad")
        self.err = errs[0]
        return dw, db


def _report(run):
    parity_report.add("footprint conv %s: workspace bytes %s" % (run.tag, ", ".join("%s %d" % kv for kv in run.ws.items())))


def _want(info, want, tag):
    assert info["family"] == want["family"], (tag, info)
    assert info["nsplit"] == want.get("nsplit", info["nsplit"]), (tag, info)
    assert (info["tail_rows"] > 0) == bool(want.get("tail")), (tag, info)


# ------------------------------------------------------------ the smallest shapes known to reach each plan family
@pytest.mark.parametrize("case", NULL_WS_CASES, ids=[c[0] for c in NULL_WS_CASES])
def test_every_plan_family_stays_inside_its_workspace(ops, case):
    """3- and 5-way K split, Winograd F(4x4,3x3), input-parity stride-2 dgrad, padded forward / dgrad, the space-to-depth
    7x7 and 3x3 stems, the K-split tail launch: the problems of NULL_WS_CASES, here WITH the workspace their query sizes."""
    name, mode, xs, ws, stride, epi_name, wino, want, _ = case
    d = ops.conv_desc(xs, ws, stride, 1, "SAME")
    ops.reset_tuning(False, False)
    prev = ops.set_winograd(wino) if wino is not None else None
    try:
        _want(ops.conv_plan_info(d, mode), want, name)
        nb = _lib().conv2d_workspace_bytes(ctypes.byref(d), mode)
        assert nb > 0, name
        run = Run(ops, d, zlib.crc32(repr(case[:5]).encode()), name)
        bound = WINO_BOUND if want["family"].startswith("winograd") else DIRECT_BOUND
        if mode == 0:
            run.fwd(tuple(epi_name.split("|")), bound)
        else:
            run.dgrad(bound, epi_names=("RESIDUAL",))
            run.dgrad(bound, epi_names=("RESIDUAL", "ACCUM"))          # the epilogue of test_null_workspace_routes_match_float64
        assert run.ws["fwd" if mode == 0 else "dgrad"] == nb
        _want(ops.conv_plan_info(d, mode), want, name)
    finally:
        if prev is not None:
            ops.set_winograd(prev)
        ops.reset_tuning()
    _report(run)


# ------------------------------------------------------------------ ragged last tiles, every tile of both engines
RAGGED = {
    # 11 RoIs of 7x7 = 539 rows (tests/row_skip): ragged against every tile height; NG = 72 / 136 against every tile width.
    # The forward and the filter gradient have NG = K, the data gradient NG = C: it runs on the transposed widths.
    "pointwise-72": ((11, 7, 7, 64), (1, 1, 64, 72), (11, 7, 7, 72), (1, 1, 72, 64)),
    "3x3-136": ((11, 7, 7, 64), (3, 3, 64, 136), (11, 7, 7, 136), (3, 3, 136, 64)),
}


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind", list(RAGGED))
def test_store_mask_of_the_last_tile(ops, kind, tile):
    """M = 539 rows is no multiple of any tile height and NG = 72 / 136 no multiple of any tile width: the last row and
    column tiles of every tile shape, on both engines, store through their masks — forward (with every epilogue), data
    gradient and filter gradient, each into NaN-prefilled guarded outputs."""
    xs, ws, xs_t, ws_t = RAGGED[kind]
    d, dt = ops.conv_desc(xs, ws, 1, 1, "SAME"), ops.conv_desc(xs_t, ws_t, 1, 1, "SAME")
    prev = ops.set_winograd(0)
    try:
        assert ops.force_conv_config(d, 0, tile) == tile and ops.force_conv_config(d, 2, tile) == tile
        assert ops.force_conv_config(dt, 1, tile) == tile
        for dd, mode, ng in ((d, 0, ws[3]), (dt, 1, ws[3]), (d, 2, ws[3])):
            info = ops.conv_plan_info(dd, mode)
            assert info["family"] == "direct" and info["code"] == tile and info["NG"] == ng, (kind, mode, info)
            # ragged against the tile in both directions (the filter gradient's rows are the 64 input channels: its
            # ragged reduction is the 539 pixels, no multiple of the 16-deep K-step)
            assert info["NG"] % info["BN"] != 0 and (info["M"] % info["BM"] != 0 or mode == 2), (kind, mode, info)
        run = Run(ops, d, zlib.crc32(kind.encode()) + tile, "%s tile %d" % (kind, tile))
        run.fwd(("BIAS", "RESIDUAL", "RELU"))
        run.wgrad(0.0)
        run_t = Run(ops, dt, zlib.crc32(kind.encode()) + 100 + tile, "%s tile %d (transposed widths)" % (kind, tile))
        run_t.dgrad()
    finally:
        ops.set_winograd(prev)
        for mode in (0, 2):
            ops.force_conv_config(d, mode, -1)
        ops.force_conv_config(dt, 1, -1)


# ---------------------------------------------------------------------------------------- the two split-K folds
@pytest.mark.parametrize("K", [18, 16], ids=["NG%4!=0-scalar-fold", "NG%4==0"])
def test_ksplit_forward_folds(ops, K):
    d = ops.conv_desc((1, 2, 2, 1024), (1, 1, 1024, K), 1, 1, "SAME")
    ops.reset_tuning(False, False)
    try:
        info = ops.conv_plan_info(d, 0)
        assert info["family"] == "direct" and info["nsplit"] == 5 and info["NG"] == K and (K % 4 != 0) == (K == 18), info
        run = Run(ops, d, 40 + K, "ksplit5 K=%d" % K)
        run.fwd()
        run.fwd(("BIAS", "RELU"))
    finally:
        ops.reset_tuning()
    _report(run)


# ------------------------------------------------------ kept transforms: the filter cache and the input transform
@pytest.mark.parametrize("shape,cfg,family,variant", [((2, 19, 23, 64, 64), 4, "winograd_F43", 0), ((11, 7, 7, 64, 64), 8, "winograd_M7", 1)],
                         ids=["F43", "whole-7-span"])
def test_kept_transforms_stay_inside_their_queries(ops, shape, cfg, family, variant):
    """The filter cache (mtlssl_conv2d_filter_xf_bytes; transform_filter on first use, the batched transform_filters on
    refresh) and the kept input transform (mtlssl_conv2d_input_xf_bytes; written by the forward, read by the filter
    gradient) are buffers the wrappers allocate themselves: GuardedOutputs guards them."""
    N, H, W, C, K = shape
    d = ops.conv_desc((N, H, W, C), (3, 3, C, K), 1, 1, "SAME")
    try:
        for mode in (0, 1, 2):
            assert ops.force_conv_config(d, mode, cfg) == cfg
            assert ops.conv_plan_info(d, mode)["family"] == family, (mode, ops.conv_plan_info(d, mode))
            assert _lib().conv2d_filter_xf_variant(ctypes.byref(d), mode) == variant
        run = Run(ops, d, 7 + cfg, family)
        cache, kept = ops.FilterXfCache(), {}
        with GuardedOutputs() as go:
            y = run.fwd(bound=WINO_BOUND, xf_cache=cache, keep_input_xf=kept)
            run.dgrad(WINO_BOUND, xf_cache=cache)
            assert len(cache.entries) == 2 and list(kept) == [run.g["x"].data_ptr()] and kept[run.g["x"].data_ptr()][1] == variant
            sizes = sorted(t.numel() * 4 for t in go.tensors)
            want = sorted([_lib().conv2d_filter_xf_bytes(ctypes.byref(d), 0), _lib().conv2d_filter_xf_bytes(ctypes.byref(d), 1),
                           _lib().conv2d_input_xf_bytes(ctypes.byref(d), variant)])
            assert sizes == want, (sizes, want)
            go.check()
            for e in cache.entries.values():
                assert bool(torch.isfinite(e["U"]).all()), "transform_filter left part of the cache unwritten"
                e["U"].fill_(float("nan"))
            cache.refresh()                                        # the batched transform rewrites every entry
            go.check()
            for e in cache.entries.values():
                assert bool(torch.isfinite(e["U"]).all()), "transform_filters left part of the cache unwritten"
            y2 = run.fwd(bound=WINO_BOUND, xf_cache=cache)
            assert torch.equal(y, y2)
            run.wgrad(0.0, WINO_BOUND, input_xf=kept[run.g["x"].data_ptr()])
            run.wgrad(1.0, WINO_BOUND, input_xf=kept[run.g["x"].data_ptr()])
            go.check()
        parity_report.add("footprint conv %s: filter cache %d B x 2, kept input transform %d B, workspace bytes %s"
                          % (family, want[0], _lib().conv2d_input_xf_bytes(ctypes.byref(d), variant),
                             ", ".join("%s %d" % kv for kv in run.ws.items())))
    finally:
        for mode in (0, 1, 2):
            ops.force_conv_config(d, mode, -1)


# ---------------------------------------------------------------------- the filter gradient in every wgrad family
WGRAD_FAMILIES = [
    # id, x shape, filter, stride, set_winograd, family conv_plan_info reports, the kernel behind it
    ("direct-multi-split", (11, 7, 7, 64), (3, 3, 64, 72), 1, 0, "direct", "tile engine, 4 splits + k_wgrad_reduce"),
    ("winograd", (1, 4, 4, 64), (3, 3, 64, 64), 1, 2, "winograd_F43", "Winograd F(4x4,3x3)"),
    ("padded", (3, 9, 11, 64), (1, 1, 64, 13), 1, None, "padded", "K zero-padded to 16 + k_wgrad_reduce_unpad"),
    ("gemm-small-pointwise", (1, 5, 7, 100), (1, 1, 100, 7), 1, None, "valu_fallback", "k_gemm_small"),
    ("stem-3-channel", (1, 16, 16, 3), (3, 3, 3, 32), 2, None, "valu_fallback", "k_conv_stem_wgrad"),
    ("scalar", (1, 16, 16, 3), (7, 7, 3, 64), 2, None, "valu_fallback", "k_conv_direct_wgrad"),
]


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("case", WGRAD_FAMILIES, ids=[c[0] for c in WGRAD_FAMILIES])
def test_filter_gradient_families(ops, case, beta):
    name, xs, ws, stride, wino, family, _ = case
    d = ops.conv_desc(xs, ws, stride, 1, "SAME")
    ops.reset_tuning(False, False)
    prev = ops.set_winograd(wino) if wino is not None else None
    try:
        info = ops.conv_plan_info(d, 2)
        assert info["family"] == family, (name, info)
        if name == "direct-multi-split":
            assert info["nsplit"] > 1, info
        # the three VALU routes are told apart by the resolver's own predicates (resolve_wgrad in csrc/conv.hip)
        pointwise, stem3 = ops.desc_is_pointwise(d), (d.R == 3 and d.S == 3 and d.C == 3 and d.K <= 64)
        if family == "valu_fallback":
            assert (pointwise, stem3) == {"gemm-small-pointwise": (True, False), "stem-3-channel": (False, True),
                                          "scalar": (False, False)}[name]
        run = Run(ops, d, zlib.crc32(name.encode()), "wgrad " + name)
        run.wgrad(beta, WINO_BOUND if family.startswith("winograd") else DIRECT_BOUND)
        assert ops.conv_plan_info(d, 2)["family"] == family
    finally:
        if prev is not None:
            ops.set_winograd(prev)
        ops.reset_tuning()
    _report(run)


# ----------------------------------------------------- row-group flags: the K-step list at the back of the workspace
@pytest.mark.parametrize("pattern", ["alternating", "none"])
def test_row_group_flags_keep_the_list_inside_the_workspace(ops, pattern):
    from tests.row_skip.test_gpu_conv_ops import PATTERNS
    d = ops.conv_desc((11, 7, 7, 64), (1, 1, 64, 128), 1, 1, "SAME")
    ops.reset_tuning(False, False)
    try:
        assert ops.set_row_skip(-1) == 1
        i1, i2 = ops.conv_plan_info(d, 1), ops.conv_plan_info(d, 2)
        assert i1["family"] == "direct" and i2["family"] == "direct" and i2["nsplit"] > 1, (i1, i2)
        run = Run(ops, d, 90, "row-skip " + pattern)
        flags = torch.tensor(PATTERNS[pattern], dtype=torch.uint8, device="cuda")
        run.set_dy((run.o["dy"] * flags.view(-1, 1, 1, 1).float()).contiguous())
        gflags = run.gs.input(flags, "active")
        run.dgrad(active=gflags, epi_names=())
        run.dgrad(active=gflags)
        dw, db = run.wgrad(0.0, active=gflags)
        run.wgrad(1.0, active=gflags)
        if pattern == "none":
            assert not bool(dw.any()) and not bool(db.any())
    finally:
        ops.set_row_skip(1)
        ops.reset_tuning()
    _report(run)


# ------------------------------------------------------------------------ the split-bf16 engine and its levels
def test_fp32_engine_modes_share_one_workspace_size(ops):
    """The smallest problem of tests/test_gpu_split_engine.py that reaches the split engine in all three passes, under
    set_fp32_engine 0..3. The filter gradient's size query is the same number in every mode, so a buffer sized in mode 0
    holds the split-engine call (the promise in wgrad_partial_bytes); which engine ran is read from engine_launches."""
    from tests.matmul_precision.test_gpu_conv_ops import BOUND
    N, H, W, C, K = 600, 7, 7, 512, 2048
    d = ops.conv_desc((N, H, W, C), (1, 1, C, K), 1, 1, "SAME")
    counter = {0: "native", 1: "six", 2: "three", 3: "one"}
    prev = ops.set_fp32_engine(0)
    try:
        for mode in (0, 1, 2):
            assert ops.force_conv_config(d, mode, 0) == 0
            assert ops.conv_plan_info(d, mode)["family"] == "direct"
        sizes = {}
        for e in (0, 1, 2, 3):
            ops.set_fp32_engine(e)
            sizes[e] = (_lib().conv2d_wgrad_workspace_bytes(ctypes.byref(d)),
                        [_lib().conv2d_workspace_bytes(ctypes.byref(d), m) for m in (0, 1, 2)])
        assert all(sizes[e] == sizes[0] for e in (1, 2, 3)), sizes
        run = Run(ops, d, 3, "fp32 engine 600x7x7x512x2048")
        native = {}
        for e in (0, 1, 2, 3):
            ops.set_fp32_engine(e)
            lim = (lambda nat: DIRECT_BOUND) if e == 0 else (lambda nat: 1.25 * max(nat, 1.0) + 2.5) if e == 1 else \
                (lambda nat, e=e: BOUND["high" if e == 2 else "medium"] + nat)
            for what, call in (("fwd", lambda b: run.fwd(("BIAS",), b)), ("dgrad", lambda b: run.dgrad(b, epi_names=())),
                               ("wgrad", lambda b: run.wgrad(0.0, b))):
                ops.engine_launches(reset=True)
                call(lim(native.get(what, 0.0)))
                counts = ops.engine_launches(reset=True)
                assert counts[counter[e]] > 0 and (e != 0 or all(v == 0 for k, v in counts.items() if k != "native")), (e, what, counts)
                if e == 0:
                    native[what] = run.err
                if what == "wgrad":
                    assert run.ws["wgrad"] == sizes[0][0], (e, run.ws, sizes[0])
            parity_report.add("footprint conv fp32 engine mode %d: workspace bytes %s" % (e, ", ".join("%s %d" % kv for kv in run.ws.items())))
    finally:
        ops.set_fp32_engine(prev)
        for mode in (0, 1, 2):
            ops.force_conv_config(d, mode, -1)


# ------------------------------------------------------------------------------ channel slices of a wider map
@pytest.mark.parametrize("shape,ws,CC,c0", [((2, 9, 11, 64), (1, 1, 64, 32), 96, 32), ((1, 13, 11, 32), (3, 3, 32, 32), 128, 32)],
                         ids=["pointwise", "3x3"])
def test_strided_slice_of_a_guarded_wide_map(ops, shape, ws, CC, c0):
    K = ws[3]
    dd, ds = ops.conv_desc(shape, ws, 1, 1, "SAME"), ops.conv_desc(shape, ws, 1, 1, "SAME", ldy=CC)
    assert ds.ldy == CC
    prev = ops.set_winograd(0)
    try:
        for mode in (0, 1):
            assert ops.conv_plan_info(ds, mode)["family"] == "direct"
        run = Run(ops, dd, CC + c0, "ldy %d" % CC)
        wide = run.gs.output((dd.N, dd.OH, dd.OW, CC), "wide y")
        run.fwd(("BIAS", "RELU"), d=ds, out=wide[..., c0:c0 + K])
        rest = torch.cat([wide[..., :c0], wide[..., c0 + K:]], -1).contiguous().view(torch.int32)
        assert bool((rest == NAN_BITS).all()), "the forward wrote outside its slice"
        g = torch.Generator(device="cuda").manual_seed(5)
        gwide = run.gs.input(torch.rand(dd.N, dd.OH, dd.OW, CC, device="cuda", generator=g) - 0.5, "wide dy")
        run.o["dy"] = gwide[..., c0:c0 + K].contiguous()
        run.dgrad(d=ds, dy=gwide[..., c0:c0 + K])
        run.wgrad(0.0, d=ds, dy=gwide[..., c0:c0 + K])
    finally:
        ops.set_winograd(prev)


# ------------------------------------------------------------------------------------ grouped / segmented calls
def test_grouped_forward_three_problems(ops):
    """mtlssl_conv2d_fwd_grouped: three problems on one input, the first a slice of a wide map; float64 at the 1e-5 of
    tests/test_gpu_conv_ops.py."""
    shape, ks, CC = (2, 19, 23, 192), (96, 48, 64), 320
    N, H, W, C = shape
    g = torch.Generator(device="cuda").manual_seed(C)
    gs = GuardSet()
    x0 = torch.randn(shape, device="cuda", generator=g)
    x = gs.input(x0, "x")
    ws = [gs.input(torch.randn(1, 1, C, k, device="cuda", generator=g) / np.sqrt(C), "w%d" % i) for i, k in enumerate(ks)]
    bs = [gs.input(torch.randn(k, device="cuda", generator=g), "bias%d" % i) for i, k in enumerate(ks)]
    wide = gs.output((N, H, W, CC), "wide y")
    outs = [wide[..., :ks[0]]] + [gs.output((N, H, W, k), "y%d" % i) for i, k in enumerate(ks[1:], 1)]
    probs = [(ops.conv_desc(shape, w.shape, 1, 1, "SAME", ldy=CC if i == 0 else 0), w, b, ops.EPI_BIAS | ops.EPI_RELU, o)
             for i, (w, b, o) in enumerate(zip(ws, bs, outs))]
    with GuardedWorkspaces() as gw:
        got = ops.conv2d_fwd_grouped(x, probs)
    gw.check()
    gs.check()
    assert bool((wide[..., ks[0]:].contiguous().view(torch.int32) == NAN_BITS).all()), "the grouped forward wrote outside its slice"
    for y, w, b, k in zip(got, ws, bs, ks):
        assert bool(torch.isfinite(y).all())
        v = (x0.reshape(-1, C).double() @ w.reshape(C, k).double() + b.double()).clamp(min=0)
        assert _relerr(y.contiguous().reshape(-1, k), v.cpu()) < 1e-5


def test_segmented_dgrad_three_segments(ops):
    shape, ks, CC, c0 = (3, 9, 11, 64), (16, 48, 32), 96, 16
    N, H, W, C = shape
    g = torch.Generator(device="cuda").manual_seed(C + 1)
    gs = GuardSet()
    ws = [gs.input(torch.randn(1, 1, C, k, device="cuda", generator=g) / np.sqrt(k), "w%d" % i) for i, k in enumerate(ks)]
    mref, res = (gs.input(torch.randn(shape, device="cuda", generator=g), n) for n in ("mask", "residual"))
    wide = gs.input(torch.randn((N, H, W, CC), device="cuda", generator=g), "wide dy")
    dys = [wide[..., c0:c0 + ks[0]]] + [gs.input(torch.randn((N, H, W, k), device="cuda", generator=g), "dy%d" % i)
                                         for i, k in enumerate(ks[1:], 1)]
    segs = [(ops.conv_desc(shape, w.shape, 1, 1, "SAME", ldy=CC if i == 0 else 0), dy, w) for i, (dy, w) in enumerate(zip(dys, ws))]
    with GuardedWorkspaces() as gw, GuardedOutputs() as go:
        dx = ops.conv2d_dgrad_segmented(segs, res, mref, ops.EPI_RESIDUAL | ops.EPI_MASK)
    gw.check()
    go.check()
    gs.check()
    assert [tuple(t.shape) for t in go.tensors] == [shape] and bool(torch.isfinite(dx).all())
    v = sum(dy.reshape(-1, k).double() @ w.reshape(C, k).double().t() for dy, w, k in zip(dys, ws, ks))
    want = (v + res.reshape(-1, C).double()) * (mref.reshape(-1, C) > 0)
    assert _relerr(dx.reshape(-1, C), want.cpu()) < 1e-5


def test_grouped_filter_gradient_three_problems(ops):
    N, H, W, C, K, R = 1, 19, 23, 64, 48, 3
    d = ops.conv_desc((N, H, W, C), (R, R, C, K), 1, 1, "SAME")
    g = torch.Generator(device="cuda").manual_seed(4)
    gs = GuardSet()
    xs = [gs.input(torch.randn(N, H, W, C, device="cuda", generator=g), "x%d" % i) for i in range(3)]
    dys = [gs.input(torch.randn(N, H, W, K, device="cuda", generator=g), "dy%d" % i) for i in range(3)]
    scales = [gs.input(torch.rand(K, device="cuda", generator=g) + 0.5, "scale%d" % i) for i in range(3)]
    for beta in (0.0, 1.0):
        old = [torch.randn(R, R, C, K, device="cuda", generator=g) for _ in range(3)]
        dws = [gs.output(None, "dw%d" % i, fill=old[i]) if beta else gs.output((R, R, C, K), "dw%d" % i) for i in range(3)]
        with GuardedWorkspaces() as gw:
            ops.conv2d_wgrad_grouped(d, xs, dys, dws, scales, beta=beta)
        gw.check()
        gs.check()
        assert gw.bytes_of("wgrad_grouped") == [_lib().conv2d_wgrad_grouped_workspace_bytes(ctypes.byref(d), 3)]
        for i in range(3):
            assert bool(torch.isfinite(dws[i]).all())
            want = old[i].clone() if beta else torch.zeros_like(old[i])       # the per-problem call, ordinary workspace
            ops.conv2d_wgrad(d, xs[i], dys[i], want, out_scale=scales[i], beta=beta)
            assert float((dws[i] - want).abs().max() / want.abs().max()) < 1e-5, (beta, i)
    parity_report.add("footprint conv grouped wgrad x3: workspace %d B" % gw.bytes_of("wgrad_grouped")[0])


# ------------------------------------------------------------------------------- depthwise wgrad, bn_param_grads
@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_filter_gradient(ops, stride):
    """N*OH*OW = 2*13*11 (stride 1) / 2*7*6 (stride 2): no multiple of the kernel's chunking; the float64 bound of
    tests/test_gpu_spatial_kernels.py."""
    from tests import spatial_ref as S
    from tests.f64_check import EPS, dev, host, within
    from tests.test_gpu_spatial_kernels import reduce_plan
    N, H, W, C = 2, 13, 11, 36
    rs = np.random.RandomState(C + stride)
    x = rs.randn(N, H, W, C).astype(np.float32)
    d = ops.conv_desc(x.shape, (3, 3, C, C), stride, 1, "SAME")
    P = N * d.OH * d.OW
    _, PL, chunks, per_chunk, depth = reduce_plan(P, C)
    assert P % per_chunk != 0 and P % PL != 0, (P, per_chunk, PL)
    gy = rs.randn(N, d.OH, d.OW, C).astype(np.float32)
    scale, prior = (rs.rand(C) + 0.5).astype(np.float32), rs.randn(3, 3, C).astype(np.float32)
    dw, sw = S.depthwise_wgrad(x, gy, stride, 1)
    gs = GuardSet()
    xg, gg, sg = gs.input(dev(x), "x"), gs.input(dev(gy), "dy"), gs.input(dev(scale), "scale")
    for beta in (0.0, 1.0):
        out = gs.output(None, "dw", fill=dev(prior)) if beta else gs.output((3, 3, C), "dw")
        with GuardedWorkspaces() as gw:
            ops.depthwise_wgrad(d, xg, gg, out, out_scale=sg, beta=beta)
        gw.check()
        gs.check()
        assert gw.bytes_of("dwgrad") == [_lib().depthwise_wgrad_workspace_bytes(ctypes.byref(d))]
        s = scale.astype(np.float64)
        ref = s * dw + beta * prior
        within(host(out), ref, (depth + 2) * EPS * s * sw + EPS * np.abs(ref), "depthwise wgrad, beta %g" % beta)
    parity_report.add("footprint depthwise wgrad stride %d: workspace %d B" % (stride, gw.bytes_of("dwgrad")[0]))


@pytest.mark.parametrize("C", [3, 4, 300, 2048])
def test_bn_param_grads(ops, C):
    """C = 3 is no multiple of 4: the library refuses it before any launch, and neither the workspace nor the outputs
    are touched. C = 4 is the narrowest map a kernel runs on."""
    from mtl_ssl_amd.lib import MtlsslError
    from tests import spatial_ref as S
    from tests.f64_check import EPS, dev, host, within
    from tests.test_gpu_spatial_kernels import reduce_plan
    rows = 2 * 19 * 27
    rs = np.random.RandomState(C)
    gamma = (rs.rand(C) + 0.5).astype(np.float32)
    beta = rs.randn(C).astype(np.float32)
    y = (rs.randn(rows, C).astype(np.float32) * gamma + beta).astype(np.float32)
    g = rs.randn(rows, C).astype(np.float32)
    prior = rs.randn(2, C).astype(np.float32)
    gs = GuardSet()
    yg, gg, gam, bet = (gs.input(dev(a), n) for a, n in ((y, "y"), (g, "g"), (gamma, "gamma"), (beta, "beta")))
    if C % 4:
        dg, db = gs.output((C,), "dgamma"), gs.output((C,), "dbeta")
        with GuardedWorkspaces() as gw:
            with pytest.raises(MtlsslError, match="multiple of 4"):
                ops.bn_param_grads(yg, gg, gam, bet, dg, db)
        gw.check()
        gs.check()
        assert bool(torch.isnan(dg).all()) and bool(torch.isnan(db).all())
        assert all(bool((b == 255).all()) for _, _, b in gw.handouts)
        return
    dgamma, dbeta, s_gy, s_g = S.bn_param_grads(y, g, gamma, beta)
    depth = reduce_plan(rows, C)[4]
    for accum in (0.0, 1.0):
        dg = gs.output(None, "dgamma", fill=dev(prior[0])) if accum else gs.output((C,), "dgamma")
        db = gs.output(None, "dbeta", fill=dev(prior[1])) if accum else gs.output((C,), "dbeta")
        with GuardedWorkspaces() as gw:
            ops.bn_param_grads(yg, gg, gam, bet, dg, db, beta=accum)
        gw.check()
        gs.check()
        assert gw.bytes_of("bngrad") == [_lib().bn_param_grads_workspace_bytes(C)]
        rg, rb = dgamma + accum * prior[0], dbeta + accum * prior[1]
        ag = np.abs(gamma.astype(np.float64))
        within(host(db), rb, depth * EPS * s_g + EPS * np.abs(rb), "dbeta, accum %g" % accum)
        within(host(dg), rg, (depth + 2) * EPS * s_gy / ag + EPS * np.abs(dgamma) + EPS * np.abs(rg), "dgamma, accum %g" % accum)
    parity_report.add("footprint bn_param_grads C=%d: workspace %d B" % (C, gw.bytes_of("bngrad")[0]))


# ----------------------------------------------------------------------------------- the instrument can fail
def test_a_torch_write_into_a_guard_is_caught():
    """The GPU half of the instrument's self-test (the CPU half is in test_host_coverage.py): one byte of this test's
    own allocation, just past the payload, written by torch."""
    import __graft_entry__ as g
    g.build()
    with GuardedWorkspaces() as gw:
        from mtl_ssl_amd import ops
        a = ops.workspace(1000, "self-test")
        b = ops.workspace(4096, "self-test")
    gw.check()
    assert gw.stats["self-test"] == [2, 5096] and a.numel() == 1000 and bool((a == 255).all())
    b.guard.parent[b.guard.parent.numel() - 512 * 1024 + 3] ^= 1
    with pytest.raises(AssertionError, match=r"workspace 'self-test', 4096 bytes: guard after the payload damaged, first at byte offset 4099"):
        gw.check()
    check_guards([a.guard])
