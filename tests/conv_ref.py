"""Float64 references and output samplers shared by the plan tests (test_gpu_plan_table.py, test_gpu_offtable_plans.py):
the reference never shortens a reduction, it samples outputs instead — flat output rows of the forward (all K channels
each) and input rows of the dgrad (all C channels), tile boundaries and image corners included, and every (r, s) tap of a
channel block of the filter gradient summed over all N*OH*OW pixels. Each returns (sum, sum |a*b|) for
tests/parity_report.py dot_err.

On top of them: fwd_expected / dgrad_expected / wgrad_expected add the epilogue's addends (to the sum AND to the scale) and
return (select, ref, mag) per compared output; ConvCase draws the operands of one problem the way every float64 plan test
does and holds the assertions they share. tests/test_conv_ref.py checks all of it on a CPU.
A plain module: no fixtures, not a conftest."""
import os
import zlib

import numpy as np
import torch

from tests.parity_report import dot_err

ROWS = 256                      # sampled rows of a forward output / dgrad input
CH = 16                         # sampled channels per side of the filter-gradient block
DIRECT_BOUND, WINO_BOUND = 8.0, 400.0       # the constants of tests/test_gpu_split_engine.py
MODE_NAMES = ("fwd", "dgrad", "wgrad")
# Worst distance of the device tanhf from the correctly rounded tanh of its own fp32 argument, in ulps of the output,
# as test_tanh_and_relu6_epilogues_at_every_site measured it on an MI355X (in the tile kernel 1.396, k_splitk_epilogue
# 1.315, k_splitk_epilogue_scalar 1.312; arguments spread over +-9.5, a quarter of the channels near 0). The assertion
# allows twice that; the margin covers arguments the cases do not sample.
TANH_ULPS_MEASURED = 1.396
TANH_ULPS = 2.0 * TANH_ULPS_MEASURED


def _rows(n_img, hs, ws, rng, n=ROWS):
    """Flat rows (img * hs + y) * ws + x to compare: 0 and M-1, both sides of the first two and the last boundary of
    every 64 / 128 / 256-row tile, the corners of the first and the last image, then random rows up to n."""
    M = n_img * hs * ws
    if M <= n:
        return np.arange(M)
    pick = {0, M - 1}
    for b in (64, 128, 256):
        for j in {1, 2, (M - 1) // b}:
            pick.update(r for r in (j * b - 1, j * b, j * b + 1) if 0 <= r < M)
    for im in (0, n_img - 1):
        for y in (0, hs - 1):
            for x in (0, ws - 1):
                pick.add((im * hs + y) * ws + x)
    rest = np.setdiff1d(np.arange(M), np.fromiter(pick, np.int64)) if M < 4 * n else None
    while len(pick) < n:
        pick.update(rng.choice(rest, n - len(pick), replace=False) if rest is not None
                    else rng.integers(0, M, n - len(pick)))
    return np.array(sorted(pick), np.int64)


def _channels(c, rng, n=CH):
    pick = {v for v in (0, 63, 64, 127, 128, 255, 256, c - 1) if v < c}
    if c <= n:
        return np.arange(c)
    rest = np.setdiff1d(np.arange(c), np.fromiter(pick, np.int64))
    pick.update(rng.choice(rest, max(n - len(pick), 0), replace=False))
    return np.array(sorted(pick), np.int64)


def _gather(t, n, y, x, valid):
    """t[n, y, x, :] for index arrays of one shape (clamped in range first), zero where not valid -> float64 CPU."""
    assert n.min() >= 0 and n.max() < t.shape[0]
    yc, xc = np.clip(y, 0, t.shape[1] - 1), np.clip(x, 0, t.shape[2] - 1)
    idx = [torch.from_numpy(np.array(a)).to(t.device) for a in (n, yc, xc)]
    g = t[idx[0], idx[1], idx[2]].double().cpu()
    return g * torch.from_numpy(valid)[..., None].double()


def _fwd_reference(prob, x, w64, rows):
    """Forward outputs of flat rows m = (n*OH + oy)*OW + ox: (sum, sum |a*b|), each [rows, K] float64."""
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    n, oy, ox = rows // (OH * OW), rows // OW % OH, rows % OW
    iy = (oy[:, None] * st - pt + np.arange(R)[None, :] * dil)[:, :, None] + np.zeros((1, 1, S), np.int64)
    ix = (ox[:, None] * st - pl + np.arange(S)[None, :] * dil)[:, None, :] + np.zeros((1, R, 1), np.int64)
    valid = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    a = _gather(x, np.broadcast_to(n[:, None, None], iy.shape), iy, ix, valid).reshape(len(rows), R * S * C)
    b = w64.reshape(R * S * C, K)
    return a @ b, a.abs() @ b.abs()


def _dgrad_reference(prob, dy, w64, rows):
    """Input gradient of flat input rows m = (n*H + iy)*W + ix: a tap (r, s) contributes where iy + pad_t - r*dil is a
    non-negative multiple of the stride whose quotient is an output row (the same along x)."""
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    n, iy, ix = rows // (H * W), rows // W % H, rows % W
    ny = iy[:, None] + pt - np.arange(R)[None, :] * dil
    nx = ix[:, None] + pl - np.arange(S)[None, :] * dil
    vy = (ny >= 0) & (ny % st == 0) & (ny // st < OH)
    vx = (nx >= 0) & (nx % st == 0) & (nx // st < OW)
    oy = (ny // st)[:, :, None] + np.zeros((1, 1, S), np.int64)
    ox = (nx // st)[:, None, :] + np.zeros((1, R, 1), np.int64)
    valid = vy[:, :, None] & vx[:, None, :]
    a = _gather(dy, np.broadcast_to(n[:, None, None], oy.shape), oy, ox, valid).reshape(len(rows), R * S * K)
    b = w64.permute(0, 1, 3, 2).reshape(R * S * K, C)
    return a @ b, a.abs() @ b.abs()


def _wgrad_reference(prob, x_sub, dy_sub):
    """sum over all N*OH*OW pixels of x[tap] * dy for a channel block: [R, S, c_sub, k_sub] (sum, sum |a*b|)."""
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    hi_y = max((OH - 1) * st - pt + (R - 1) * dil - (H - 1), 0)
    hi_x = max((OW - 1) * st - pl + (S - 1) * dil - (W - 1), 0)
    xp = torch.nn.functional.pad(x_sub, (0, 0, pl, hi_x, pt, hi_y))       # zeros where a tap reads the padding
    g = dy_sub.reshape(-1, dy_sub.shape[-1])
    ref = torch.empty(R, S, x_sub.shape[-1], g.shape[1], dtype=torch.float64)
    mag = torch.empty_like(ref)
    for r in range(R):
        for s in range(S):
            a = xp[:, r * dil:r * dil + (OH - 1) * st + 1:st, s * dil:s * dil + (OW - 1) * st + 1:st, :]
            assert a.shape[1:3] == (OH, OW)
            a = a.reshape(-1, a.shape[-1])
            ref[r, s], mag[r, s] = a.t() @ g, a.abs().t() @ g.abs()
    return ref, mag


# ------------------------------------------------------- expected values: a reference plus the epilogue's addends
def _np(v):
    return v.numpy() if torch.is_tensor(v) else np.asarray(v)


def _idx(a, like):
    return None if a is None else torch.from_numpy(np.asarray(a, np.int64)).to(like.device)


def _tuple(outs):
    return outs if isinstance(outs, tuple) else (outs,)


def _plus(ref, mag, *addends):
    """Every addend of the epilogue goes into the reference and, by its magnitude, into the unit of the error."""
    for a in addends:
        if a is not None:
            ref, mag = ref + a, mag + a.abs()
    return ref, mag


def _picker(width, rows, cols, like):
    """(column index or None, select) of a [..., width] map: its flat rows `rows`, of those the columns `cols` (None: all)."""
    r, c = _idx(rows, like), _idx(cols, like)
    if c is None:
        return c, lambda t: t.contiguous().reshape(-1, width)[r]
    return c, lambda t: t.contiguous().reshape(-1, width)[r][:, c]


def fwd_expected(prob, x, w, rows, cols=None, bias=None, res=None, relu=False):
    """The forward on flat output rows `rows`, on all K columns or on the subset `cols` (the float64 filter is then built
    for those alone: the problem prob[:4] + (len(cols),) + prob[5:]), plus bias and residual, through a ReLU if `relu`
    (|relu(a) - relu(b)| <= |a - b|: the scale stays). -> (select, ref, mag); select maps the kernel's y to the samples."""
    c, sel = _picker(prob[4], rows, cols, x)
    if c is not None:
        prob, w, bias = prob[:4] + (len(cols),) + prob[5:], w[..., c], None if bias is None else bias[c]
    ref, mag = _fwd_reference(prob, x, w.double().cpu(), rows)
    ref, mag = _plus(ref, mag, None if bias is None else bias.double().cpu()[None, :], None if res is None else sel(res).double().cpu())
    return sel, (torch.relu(ref) if relu else ref), mag


def dgrad_expected(prob, dy, w, rows, cols=None, resd=None, prev=None, mask=None):
    """The data gradient on flat input rows `rows` (columns as in fwd_expected: prob[:3] + (len(cols),) + prob[4:]) plus the
    residual gradient and the previous contents it accumulates into. Behind the ReLU mask (`mask` > 0 passes) a masked
    sample is exactly 0: ref * on, and its scale is 1 so that any nonzero value there is an error. -> (select, ref, mag)."""
    c, sel = _picker(prob[3], rows, cols, dy)
    if c is not None:
        prob, w = prob[:3] + (len(cols),) + prob[4:], w[:, :, c, :]
    ref, mag = _dgrad_reference(prob, dy, w.double().cpu(), rows)
    ref, mag = _plus(ref, mag, *(None if t is None else sel(t).double().cpu() for t in (resd, prev)))
    if mask is not None:
        on = (sel(mask) > 0).cpu()
        ref, mag = ref * on, torch.where(on, mag, torch.ones_like(mag))
    return sel, ref, mag


def wgrad_expected(prob, x, dy, cs, ks, scale=None, beta=1.0, dw_old=None, db_old=None):
    """The filter gradient on the channel block cs x ks, beta * dw_old + scale * sum, and the bias gradient on ks,
    beta * db_old + the column sum of dy (never scaled). -> (select, ref, mag) of dw, (select, ref, mag) of db."""
    c, k = _idx(cs, x), _idx(ks, x)
    sel_w, sel_b = (lambda t: t[:, :, c][..., k]), (lambda t: t[k])
    old = lambda t, sel: None if t is None else beta * sel(t).double().cpu()
    dy_sub = dy[..., k].double().cpu()
    ref, mag = _wgrad_reference(prob, x[..., c].double().cpu(), dy_sub)
    if scale is not None:
        s64 = scale[k].double().cpu()
        ref, mag = s64 * ref, s64.abs() * mag
    return ((sel_w,) + _plus(ref, mag, old(dw_old, sel_w)),
            (sel_b,) + _plus(dy_sub.sum((0, 1, 2)), dy_sub.abs().sum((0, 1, 2)), old(db_old, sel_b)))


def fp32_spacing(v64):
    """The spacing of fp32 at |v| (float64 in and out)."""
    return np.spacing(np.maximum(np.abs(_np(v64)), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def fp32_ulps(got, ref64):
    """|got - ref| in units of the fp32 spacing at |ref| (float64 arrays)."""
    return np.abs(got - ref64) / fp32_spacing(ref64)


def tanh_tolerance(mag, at, bound):
    """What a forward output behind the TANH epilogue may differ from tanh of the float64 linear reference: the linear
    bound (tanh' <= 1, so it carries over) plus TANH_ULPS fp32 spacings at the tanh value `at`. A float64 array."""
    return bound * 2.0 ** -24 * _np(mag) + TANH_ULPS * fp32_spacing(at)


# --------------------------------------------------------------------------------- small parts the plan tests share
def pid(prob, mode=None, name=None):
    """Test id of a problem; with `mode` its name in front; with `name` (the VGG lists) the short form behind name[:4]."""
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    if name is not None:
        return "%s-%s-%dx%dx%dx%d-k%d-%dx%d" % (name[:4], MODE_NAMES[mode], N, H, W, C, K, R, S)
    s = "%dx%dx%dx%d-k%d-%dx%d-o%dx%d-s%dd%dp%d%d" % (N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl)
    return s if mode is None else MODE_NAMES[mode] + "-" + s


def prob_of(d):
    return (d.N, d.H, d.W, d.C, d.K, d.R, d.S, d.OH, d.OW, d.stride, d.dilation, d.pad_t, d.pad_l)


def family_lines(run):
    """Report lines, one per plan family, of (family, mode, error) records: cases and worst error per mode."""
    fams = {}
    for fam, mode, err in run:
        f = fams.setdefault(fam, [[0, 0.0], [0, 0.0], [0, 0.0]])
        f[mode][0] += 1
        f[mode][1] = max(f[mode][1], err)
    return ["    %-16s %d / %d / %d cases; worst error in 2^-24*sum|ab| units %s" % (
        name, f[0][0], f[1][0], f[2][0], " / ".join("%.2f" % v[1] for v in f)) for name, f in sorted(fams.items())]


def plan_test_ops(planning_switches=None):
    """The body of the plan tests' module-scoped `ops` fixture (each module wraps it in its own @pytest.fixture): the built
    package on poisoned workspaces, the native fp32 engine, the plan table on and the tuner off; both restored after."""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    assert ops.POISON_WS, "the suite runs with NaN-poisoned workspaces (tests/conftest.py)"
    if planning_switches is not None:
        assert not [k for k in planning_switches if k in os.environ], "a planning switch is set"
    prev = ops.set_fp32_engine(0)
    ops.reset_tuning(use_plan_db=True, autotune=False)
    yield ops
    ops.set_fp32_engine(prev)
    ops.reset_tuning()


class ConvCase:
    """One problem of a float64 plan test: the generator (seeded with crc32(repr(prob)) unless a seed is given), the
    numpy rng of the samples, and the operands — post-ReLU-like x, a zero-mean w scaled by 2/sqrt(RSC), zero-mean dy,
    drawn here; a mode's extras, its sample and its expected values when prepare(mode) asks for them."""

    def __init__(self, prob, seed=None, device="cuda"):
        self.prob = prob = tuple(prob)
        N, H, W, C, K, R, S, OH, OW = prob[:9]
        seed = zlib.crc32(repr(prob).encode()) if seed is None else seed
        self.gen, self.rng = torch.Generator(device=device).manual_seed(seed), np.random.default_rng(seed)
        self.rand = lambda *shape: torch.rand(*shape, device=device, generator=self.gen)
        self.x = self.rand(N, H, W, C) * 2 - 0.6                            # post-ReLU-like: mostly positive
        self.w = (self.rand(R, S, C, K) - 0.5) * (2.0 / np.sqrt(R * S * C))
        self.dy = self.rand(N, OH, OW, K) - 0.5                             # zero-mean
        self.sample, self.expected = {}, {}     # mode -> (rows, cols) / (cs, ks); mode -> [(select, ref, mag)] per output

    def prepare(self, mode, rows=_rows, cols=None, res=True, relu=False):
        """Draws the extras of the mode (0: bias, res; 1: resd, prev, mask; 2: scale, dw_old, db_old), then its sample,
        rows(n_img, hs, ws, rng) before cols(width, rng) (None: every column), cs before ks, and builds expected[mode]:
        forward with bias and residual (`res` False: no residual drawn), dgrad with the residual accumulated into prev,
        wgrad with out_scale, dbias and beta = 1."""
        N, H, W, C, K, R, S, OH, OW = self.prob[:9]
        rand, rng = self.rand, self.rng
        if mode == 0:
            self.bias, self.res = rand(K) - 0.5, (rand(N, OH, OW, K) - 0.5 if res else None)
            s = self.sample[0] = (rows(N, OH, OW, rng), cols and cols(K, rng))
            self.expected[0] = [fwd_expected(self.prob, self.x, self.w, s[0], s[1], self.bias, self.res, relu)]
        elif mode == 1:
            self.resd, self.prev, self.mask = (rand(N, H, W, C) - 0.5 for _ in range(3))
            s = self.sample[1] = (rows(N, H, W, rng), cols and cols(C, rng))
            self.expected[1] = [dgrad_expected(self.prob, self.dy, self.w, s[0], s[1], self.resd, self.prev)]
        else:
            self.scale, self.dw_old, self.db_old = rand(K) + 0.5, rand(R, S, C, K) - 0.5, rand(K) - 0.5
            s = self.sample[2] = (_channels(C, rng), _channels(K, rng))
            self.expected[2] = list(wgrad_expected(self.prob, self.x, self.dy, s[0], s[1], self.scale, 1.0, self.dw_old, self.db_old))

    def call(self, ops, d, mode, nonlinear=False, **kw):
        """The launch prepare(mode) expects; `nonlinear` adds the ReLU to the forward, the ReLU mask to the dgrad."""
        if mode == 0:
            return ops.conv2d_fwd(d, self.x, self.w, self.bias, self.res,
                                  ops.EPI_BIAS | ops.EPI_RESIDUAL | (ops.EPI_RELU if nonlinear else 0), **kw)
        if mode == 1:
            dx = self.prev.clone()
            ops.conv2d_dgrad(d, self.dy, self.w, self.resd, self.mask if nonlinear else None,
                             ops.EPI_RESIDUAL | ops.EPI_ACCUM | (ops.EPI_MASK if nonlinear else 0), out=dx, **kw)
            return dx
        dw, db = self.dw_old.clone(), self.db_old.clone()
        ops.conv2d_wgrad(d, self.x, self.dy, dw, out_scale=self.scale, dbias=db, beta=1.0, **kw)
        return dw, db

    def check_finite(self, outs, *ctx):
        for t in _tuple(outs):
            assert bool(torch.isfinite(t).all()), ("non-finite output (a poisoned workspace leaked?)",) + ctx

    def errors(self, mode, outs):
        """dot_err of every output of the mode (y / dx / dw, db) on its samples."""
        return [dot_err(sel(o), ref, mag) for o, (sel, ref, mag) in zip(_tuple(outs), self.expected[mode])]

    def check_errors(self, mode, outs, bound, tag, note=None):
        """The first output within the plan family's `bound`, the rest (the bias gradient: a plain column sum) within
        DIRECT_BOUND. note(errs, lims) — the caller's print and record — runs before the assertion. -> errs."""
        errs = self.errors(mode, outs)
        lims = [bound] + [DIRECT_BOUND] * (len(errs) - 1)
        if note is not None:
            note(errs, lims)
        assert all(e <= lim for e, lim in zip(errs, lims)), (MODE_NAMES[mode], tag, errs, lims)
        return errs

    def check_exact_epilogue(self, mode, got, linear, *ctx):
        """The nonlinear epilogues are exact functions of the linear result (the split-K fold sums in a fixed order)."""
        if mode == 0:
            assert torch.equal(got, torch.relu(linear)), ("forward ReLU epilogue",) + ctx
        if mode == 1:
            assert torch.equal(got, torch.where(self.mask > 0, linear, torch.zeros_like(linear))), ("dgrad mask epilogue",) + ctx

