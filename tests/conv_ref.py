"""Float64 references shared by the plan tests (test_gpu_plan_table.py, test_gpu_offtable_plans.py,
vgg/test_gpu_fullsize_plans.py). Two of them, and neither shortens a reduction:

  * whole (fwd / dgrad / wgrad_reference_whole): EVERY output element, by a plain tap walk of the operands cast to float64
    on the device the operands live on — x zero-padded once, per tap (r, s) one strided slice times w[r, s], in row chunks
    of at most 2 GiB — compared on that device by dot_err_whole, which returns the worst error and where it is; locate()
    turns the index into row, column, tile and split. This is the comparison that covers the output.
  * sampled (_fwd / _dgrad / _wgrad_reference), built on the CPU: ~256 flat output rows of the forward (all K channels
    each) and input rows of the dgrad (all C channels), tile boundaries and image corners included, and every (r, s) tap
    of a 16 x 16 channel block of the filter gradient summed over all N*OH*OW pixels. It stays for two reasons: it is the
    independent yardstick of the whole one (the device's float64 matmul is a library kernel on a new chip: ConvCase.
    reference_difference holds the two to n * 2^-52 * scale on the sample), and its numbers are the parity report's
    series since the plan tests exist.

Each returns (sum, sum |a*b|), the unit of tests/parity_report.py dot_err.

On top of them: fwd_expected / dgrad_expected / wgrad_expected add the epilogue's addends (to the sum AND to the scale) and
return (select, ref, mag) per compared output; ConvCase draws the operands of one problem the way every float64 plan test
does and holds the assertions they share. apply_fwd_epilogue / apply_dgrad_epilogue are the epilogue flags' two chains in
fp32 torch, what a flagged output must equal bit for bit given the unflagged one (csrc/epilogue.h states them for the
kernels). tests/test_conv_ref.py checks all of it on a CPU.
A plain module: no fixtures, not a conftest."""
import os
import zlib

import numpy as np
import torch

from tests.parity_report import dot_err

ROWS = 256                      # sampled rows of a forward output / dgrad input
CH = 16                         # sampled channels per side of the filter-gradient block
# The constants of tests/test_gpu_split_engine.py, set on samples. They hold over every output element as they are
# (profiles/whole_output_observed.txt, one MI355X): 2.71e9 elements of the plan table's 359 pairs, worst direct 7.07 (on the
# sample 5.29), worst Winograd 47.06 (34.22), worst bias gradient 1.43; no element beyond either bound, so neither has a
# whole-output limit of its own.
DIRECT_BOUND, WINO_BOUND = 8.0, 400.0
MODE_NAMES = ("fwd", "dgrad", "wgrad")
WHOLE_BYTES = 2 << 30           # no float64 temporary of a whole-output reference is larger
ERR_CHUNK = 1 << 26             # elements of an output compared at a time (dot_err_whole)
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


# ------------------------------------------------------------- whole outputs: the same sums for every element, on `device`
def _pad_hi(prob):
    """Rows / columns of zeros below / right of x that the last output row / column reads."""
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    return max((OH - 1) * st - pt + (R - 1) * dil - (H - 1), 0), max((OW - 1) * st - pl + (S - 1) * dil - (W - 1), 0)


def _chunks(prob):
    """Output row chunks (n0, n1, y0, y1) — whole images, or row ranges of one image where one image is too large — such
    that no float64 temporary of a tap walk (the padded x, a tap's [rows, C] slice, a [rows, K] product) exceeds WHOLE_BYTES.
    The flat output rows of a chunk are contiguous: (n0*OH + y0)*OW up to (n0*OH + y0)*OW + (n1-n0)*(y1-y0)*OW."""
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    hi_y, hi_x = _pad_hi(prob)
    limit = WHOLE_BYTES // 8
    wp = (W + pl + hi_x) * C
    per_img = max((H + pt + hi_y) * wp, OH * OW * max(C, K))
    if per_img <= limit:
        step = max(limit // per_img, 1)
        return [(n0, min(n0 + step, N), 0, OH) for n0 in range(0, N, step)]
    ystep = max(limit // max(OW * max(C, K), (st + (R - 1) * dil) * wp), 1)
    return [(n, n + 1, y0, min(y0 + ystep, OH)) for n in range(N) for y0 in range(0, OH, ystep)]


def _padded(x, prob, chunk, device, dtype):
    """x of the chunk's images in `dtype` on `device`, zero-padded once, cut to the rows the chunk's output rows read:
    its row j is input row y0*stride - pad_t + j, its column i input column i - pad_l."""
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    n0, n1, y0, y1 = chunk
    lo, hi = y0 * st - pt, (y1 - 1) * st - pt + (R - 1) * dil           # first and last input row read
    a = min(max(lo, 0), H)
    b = max(min(hi, H - 1) + 1, a)
    xs = x[n0:n1, a:b].to(device=device, dtype=dtype)
    return torch.nn.functional.pad(xs, (0, 0, pl, _pad_hi(prob)[1], a - lo, hi + 1 - b))


def _tap(t, prob, r, s, y0, y1):
    """The strided slice of a padded map that tap (r, s) pairs with output rows y0..y1 (t's row 0 is padded row y0*stride)."""
    OH, OW, st, dil = prob[7], prob[8], prob[9], prob[10]
    a = t[:, r * dil:r * dil + (y1 - y0 - 1) * st + 1:st, s * dil:s * dil + (OW - 1) * st + 1:st, :]
    assert a.shape[1:3] == (y1 - y0, OW)
    return a


def fwd_reference_whole(prob, operands, device, dtype=torch.float64):
    """Every forward output by a plain tap walk of operands = (x, w) cast to `dtype`: x zero-padded once per chunk, for
    each tap (r, s) its strided slice as [rows, C] times w[r, s]. -> (sum, sum |a*b|), each [N*OH*OW, K] on `device`."""
    x, w = operands
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    wd = w.to(device=device, dtype=dtype)
    wa = wd.abs()
    ref = torch.zeros(N * OH * OW, K, dtype=dtype, device=device)
    mag = torch.zeros_like(ref)
    for chunk in _chunks(prob):
        n0, n1, y0, y1 = chunk
        xp = _padded(x, prob, chunk, device, dtype)
        m0 = (n0 * OH + y0) * OW
        m1 = m0 + (n1 - n0) * (y1 - y0) * OW
        for r in range(R):
            for s in range(S):
                a = _tap(xp, prob, r, s, y0, y1).reshape(-1, C)
                ref[m0:m1].addmm_(a, wd[r, s])
                mag[m0:m1].addmm_(a.abs(), wa[r, s])
    return ref, mag


def dgrad_reference_whole(prob, operands, device, dtype=torch.float64):
    """Every input gradient by the adjoint of that walk: operands = (dy, w); for each tap dy @ w[r, s].T is added into the
    tap's strided slice of a zero-padded dx, which is cropped at the end. -> (sum, sum |a*b|), each [N*H*W, C]."""
    dy, w = operands
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    hi_y, hi_x = _pad_hi(prob)
    wd = w.to(device=device, dtype=dtype)
    wa = wd.abs()
    ref = torch.zeros(N, pt + H + hi_y, pl + W + hi_x, C, dtype=dtype, device=device)
    mag = torch.zeros_like(ref)
    for n0, n1, y0, y1 in _chunks(prob):
        g = dy[n0:n1, y0:y1].to(device=device, dtype=dtype).reshape(-1, K)
        ga = g.abs()
        for r in range(R):
            for s in range(S):
                shape = (n1 - n0, y1 - y0, OW, C)
                _tap(ref[n0:n1, y0 * st:], prob, r, s, y0, y1).add_((g @ wd[r, s].t()).reshape(shape))
                _tap(mag[n0:n1, y0 * st:], prob, r, s, y0, y1).add_((ga @ wa[r, s].t()).reshape(shape))
    crop = lambda t: t[:, pt:pt + H, pl:pl + W, :].reshape(N * H * W, C)
    return crop(ref), crop(mag)


def wgrad_reference_whole(prob, operands, device, dtype=torch.float64):
    """Every filter gradient element: operands = (x, dy); per tap a.T @ g over all N*OH*OW pixels (what _wgrad_reference
    does for a channel block). -> (sum, sum |a*b|), each [R, S, C, K]."""
    x, dy = operands
    N, H, W, C, K, R, S, OH, OW, st, dil, pt, pl = prob
    ref = torch.zeros(R, S, C, K, dtype=dtype, device=device)
    mag = torch.zeros_like(ref)
    for chunk in _chunks(prob):
        n0, n1, y0, y1 = chunk
        xp = _padded(x, prob, chunk, device, dtype)
        g = dy[n0:n1, y0:y1].to(device=device, dtype=dtype).reshape(-1, K)
        ga = g.abs()
        for r in range(R):
            for s in range(S):
                a = _tap(xp, prob, r, s, y0, y1).reshape(-1, C)
                ref[r, s].addmm_(a.t(), g)
                mag[r, s].addmm_(a.abs().t(), ga)
    return ref, mag


def dbias_reference_whole(prob, dy, device, dtype=torch.float64):
    """The bias gradient, the column sum of dy over all pixels. -> (sum, sum |dy|), each [K]."""
    K = prob[4]
    ref = torch.zeros(K, dtype=dtype, device=device)
    mag = torch.zeros_like(ref)
    for n0, n1, y0, y1 in _chunks(prob):
        g = dy[n0:n1, y0:y1].to(device=device, dtype=dtype).reshape(-1, K)
        ref += g.sum(0)
        mag += g.abs().sum(0)
    return ref, mag


def _err_chunks(y, ref, mag):
    """(offset, errors) over flat chunks of an output: |y - ref| in units of 2^-24 * mag on the reference's device; where
    the scale is 0 the error is 0 for an exact 0 and infinite for anything else, as it is for a NaN anywhere."""
    yf, rf, mf = y.reshape(-1), ref.reshape(-1), mag.reshape(-1)
    assert yf.numel() == rf.numel() == mf.numel(), (y.shape, ref.shape, mag.shape)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=rf.device)
    for o in range(0, rf.numel(), ERR_CHUNK):
        yd, r, m = yf[o:o + ERR_CHUNK].to(rf.device).double(), rf[o:o + ERR_CHUNK].double(), mf[o:o + ERR_CHUNK].double()
        err = torch.where(m > 0, (yd - r).abs() / (m * 2.0 ** -24), torch.where(yd == 0, torch.zeros_like(inf), inf))
        yield o, torch.nan_to_num(err, nan=float("inf"), posinf=float("inf"))


def dot_err_whole(y, ref, mag):
    """tests/parity_report.py dot_err over every element without a host copy of the output: the worst |y - ref| in units of
    2^-24 * mag and the flat index of that element. An output with scale 0 that is not exactly 0 (or one that is not a
    number) makes the error infinite instead of raising, so that the caller can say where it is."""
    worst, at = 0.0, 0
    for o, err in _err_chunks(y, ref, mag):
        v, i = err.max(0)
        if float(v) > worst:
            worst, at = float(v), o + int(i)
    return worst, at


def worst_whole(y, ref, mag, bound, k=20):
    """The k worst elements of an output as [(error, flat index)], worst first, and the number of elements beyond `bound`."""
    top, beyond = [], 0
    for o, err in _err_chunks(y, ref, mag):
        beyond += int((err > bound).sum())
        v, i = err.topk(min(k, err.numel()))
        top += [(float(a), o + int(b)) for a, b in zip(v, i)]
    return sorted(top, reverse=True)[:k], beyond


def locate(prob, mode, which, idx, info=None, sub_info=None):
    """What flat index `idx` of an output means: of y / dx (which 0) the flat row, its image and pixel and the column; of dw
    the tap, the row (input channel) and the column (output channel); of db (which 1) the column. With the plan's
    ops.conv_plan_info `info` also the BM x BN tile of the GEMM it lies in and, for a K-split plan, the split that sums it
    (of the main or the tail launch). `sub_info(parity class)` gives the sub-problem plans of an input-parity dgrad."""
    N, H, W, C, K, R, S, OH, OW = prob[:9]
    tile = lambda i, row, col: "" if not i or i["BM"] <= 0 or i["BN"] <= 0 else ", %dx%d tile (%d, %d) of the %d x %d GEMM" % (
        i["BM"], i["BN"], row // i["BM"], col // i["BN"], i["M"], i["NG"])
    if mode == 2 and which == 1:
        return "db column %d" % idx
    if mode == 2:
        k, c, s, r = idx % K, idx // K % C, idx // (K * C) % S, idx // (K * C * S)
        text = "dw tap (%d, %d), row %d, column %d" % (r, s, c, k)
        if info and (info["M"], info["NG"]) == (C, K):
            text += tile(info, c, k)
            if info["nsplit"] > 1:
                text += ", summed over %d splits of %d pixels" % (info["nsplit"], info["pix_per_split"])
        return text
    (hs, ws, width), name = ((OH, OW, K), "y") if mode == 0 else ((H, W, C), "dx")
    row, col = idx // width, idx % width
    n, py, px = row // (hs * ws), row // ws % hs, row % ws
    text = "%s row %d, column %d (image %d, pixel %d, %d)" % (name, row, col, n, py, px)
    if not info:
        return text
    if info["family"] == "input_parity" and sub_info is not None:
        cy, cx = py & 1, px & 1
        h2, w2 = (hs - cy + 1) // 2, (ws - cx + 1) // 2
        info, row = sub_info(cy * 2 + cx), (n * h2 + py // 2) * w2 + px // 2
        text += ", parity class %d row %d" % (cy * 2 + cx, row)
    elif info["M"] != N * hs * ws:
        return text + ("" if info["BM"] <= 0 else ", plan %s runs a %d x %d GEMM in %dx%d tiles" % (
            info["family"], info["M"], info["NG"], info["BM"], info["BN"]))
    text += tile(info, row, col)
    if info["BM"] > 0 and info["tail_rows"] > 0 and row >= (-(-info["M"] // info["BM"]) - info["tail_rows"]) * info["BM"]:
        text += ", K-split tail launch: %d splits of %d K-steps" % (info["tail_nsplit"], info["tail_ks"])
    elif info["nsplit"] > 1:
        text += ", K split: %d splits of %d of %d K-steps" % (info["nsplit"], info["ks_per_split"], info["ksteps"])
    return text


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


def apply_fwd_epilogue(lin, epi, bias=None, res=None):
    """The forward epilogue (ops.EPI_* flags) on a linear result `lin`, in fp32 torch and in the library's order:
    (lin + bias) + res under BIAS / RESIDUAL, then RELU as max(., 0), RELU6 as clamp(., 0, 6). TANH is the float64 tanh of
    that fp32 pre-activation, returned in float64: the device tanhf is held to it in fp32 spacings (TANH_ULPS)."""
    from mtl_ssl_amd import ops as O
    v = lin
    if epi & O.EPI_BIAS:
        v = v + bias
    if epi & O.EPI_RESIDUAL:
        v = v + res
    if epi & O.EPI_RELU:
        v = torch.clamp_min(v, 0.0)
    if epi & O.EPI_RELU6:
        v = torch.clamp(v, 0.0, 6.0)
    if epi & O.EPI_TANH:
        v = torch.tanh(v.double())
    return v


def apply_dgrad_epilogue(lin, epi, resd=None, prev=None, mask_ref=None):
    """The input-gradient epilogue on a linear result, in fp32 torch and in the library's order: (lin + resd) + prev
    under RESIDUAL / ACCUM, then 0 wherever the activation that made `mask_ref` was not in its linear range: MASK
    passes mask_ref > 0, MASK6 0 < mask_ref < 6."""
    from mtl_ssl_amd import ops as O
    v = lin
    if epi & O.EPI_RESIDUAL:
        v = v + resd
    if epi & O.EPI_ACCUM:
        v = v + prev
    if epi & (O.EPI_MASK | O.EPI_MASK6):
        on = mask_ref > 0
        if epi & O.EPI_MASK6:
            on = on & (mask_ref < 6)
        v = torch.where(on, v, torch.zeros_like(v))
    return v


def _on(device, dtype, *ts):
    return [None if t is None else t.to(device=device, dtype=dtype) for t in ts]


def fwd_expected_whole(prob, x, w, device, bias=None, res=None, relu=False, dtype=torch.float64):
    """fwd_expected for every output element, on `device`. -> (ref, mag), each [N*OH*OW, K]."""
    bias, res = _on(device, dtype, bias, res)
    ref, mag = fwd_reference_whole(prob, (x, w), device, dtype)
    ref, mag = _plus(ref, mag, None if bias is None else bias[None, :], None if res is None else res.reshape(ref.shape))
    return (torch.relu(ref) if relu else ref), mag


def dgrad_expected_whole(prob, dy, w, device, resd=None, prev=None, mask=None, dtype=torch.float64):
    """dgrad_expected for every input element (a masked one exactly 0 on scale 1). -> (ref, mag), each [N*H*W, C]."""
    ref, mag = dgrad_reference_whole(prob, (dy, w), device, dtype)
    ref, mag = _plus(ref, mag, *(None if t is None else t.reshape(ref.shape) for t in _on(device, dtype, resd, prev)))
    if mask is not None:
        on = (mask.to(device) > 0).reshape(ref.shape)
        ref, mag = ref * on, torch.where(on, mag, torch.ones_like(mag))
    return ref, mag


def wgrad_expected_whole(prob, x, dy, device, scale=None, beta=1.0, dw_old=None, db_old=None, dtype=torch.float64):
    """wgrad_expected for every element. -> (ref, mag) of dw [R, S, C, K], (ref, mag) of db [K]."""
    scale, dw_old, db_old = _on(device, dtype, scale, dw_old, db_old)
    ref, mag = wgrad_reference_whole(prob, (x, dy), device, dtype)
    if scale is not None:
        ref, mag = scale * ref, scale.abs() * mag
    old = lambda t: None if t is None else beta * t
    return _plus(ref, mag, old(dw_old)), _plus(*dbias_reference_whole(prob, dy, device, dtype), old(db_old))


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
    """Report lines, one per plan family, of (family, mode, error) records: cases and worst sampled error per mode. A
    record that goes on with (whole-output worst error, elements compared, worst device-vs-CPU reference difference) adds
    a second line to its family (whole_line)."""
    fams, whole = {}, {}
    for fam, mode, err, *rest in run:
        f = fams.setdefault(fam, [[0, 0.0], [0, 0.0], [0, 0.0]])
        f[mode][0] += 1
        f[mode][1] = max(f[mode][1], err)
        if rest:
            whole.setdefault(fam, []).append((mode,) + tuple(rest))
    lines = []
    for name, f in sorted(fams.items()):
        lines.append("    %-16s %d / %d / %d cases; worst error in 2^-24*sum|ab| units %s" % (
            name, f[0][0], f[1][0], f[2][0], " / ".join("%.2f" % v[1] for v in f)))
        if name in whole:
            lines.append(whole_line(whole[name]))
    return lines


def whole_line(records):
    """Report line of (mode, whole-output worst error, elements compared, reference difference) records of one family."""
    worst, elements, diff = [0.0, 0.0, 0.0], [0, 0, 0], 0.0
    for mode, err, n, d in records:
        worst[mode], elements[mode], diff = max(worst[mode], err), elements[mode] + n, max(diff, d)
    return ("        every output element: %s elements compared; worst error %s; float64 reference on the device against "
            "the CPU's on the sample: worst %.3f of n*2^-52*scale" % (
                " / ".join("%d" % n for n in elements), " / ".join("%.2f" % v for v in worst), diff))


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
        self.whole, self.whole_stats = {}, {}   # mode -> [(ref, mag)] per output, whole and on the device; mode -> figures
        self.relu = False

    def prepare(self, mode, rows=_rows, cols=None, res=True, relu=False):
        """Draws the extras of the mode (0: bias, res; 1: resd, prev, mask; 2: scale, dw_old, db_old), then its sample,
        rows(n_img, hs, ws, rng) before cols(width, rng) (None: every column), cs before ks, and builds expected[mode]:
        forward with bias and residual (`res` False: no residual drawn), dgrad with the residual accumulated into prev,
        wgrad with out_scale, dbias and beta = 1."""
        N, H, W, C, K, R, S, OH, OW = self.prob[:9]
        rand, rng = self.rand, self.rng
        if mode == 0:
            self.bias, self.res, self.relu = rand(K) - 0.5, (rand(N, OH, OW, K) - 0.5 if res else None), relu
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

    def prepare_whole(self, mode, dtype=torch.float64):
        """After prepare(mode), and drawing nothing: the expected value and its scale of EVERY element of the mode's
        outputs, [(ref, mag)] per output on the operands' device, from the operands and extras prepare(mode) drew. Kept
        as whole[mode] in float64; in another dtype (float32: the plain evaluation a rounding tail is measured by) only
        returned."""
        p, dev = self.prob, self.x.device
        if mode == 0:
            out = [fwd_expected_whole(p, self.x, self.w, dev, self.bias, self.res, self.relu, dtype)]
        elif mode == 1:
            out = [dgrad_expected_whole(p, self.dy, self.w, dev, self.resd, self.prev, dtype=dtype)]
        else:
            out = list(wgrad_expected_whole(p, self.x, self.dy, dev, self.scale, 1.0, self.dw_old, self.db_old, dtype))
        if dtype == torch.float64:
            self.whole[mode] = out
        return out

    def reference_difference(self, mode):
        """Pins the device's float64 matmul, a library kernel: the whole reference (and its scale) on the sample against
        the CPU reference of prepare(mode). Two float64 summation orders of n exact products differ by at most
        n * 2^-52 * sum|ab| to first order, n the reduction length — asserted per element. -> the worst ratio to it."""
        N, H, W, C, K, R, S, OH, OW = self.prob[:9]
        n, worst = (R * S * C, R * S * K, N * OH * OW)[mode], 0.0
        for (ref_w, mag_w), (sel, ref, mag) in zip(self.whole[mode], self.expected[mode]):
            tol = n * 2.0 ** -52 * mag
            for what, a, b in (("sum", ref_w, ref), ("scale", mag_w, mag)):
                diff = (sel(a).cpu() - b).abs()
                assert bool((diff <= tol).all()), ("float64 reference on the device against the CPU's", MODE_NAMES[mode], what,
                                                  float((diff / tol.clamp_min(1e-300)).max()))
                if bool((tol > 0).any()):
                    worst = max(worst, float((diff[tol > 0] / tol[tol > 0]).max()))
        return worst

    def whole_errors(self, mode, outs):
        """dot_err_whole of every output of the mode: [(worst error, flat index)]."""
        if mode not in self.whole:
            self.prepare_whole(mode)
        return [dot_err_whole(o, ref, mag) for o, (ref, mag) in zip(_tuple(outs), self.whole[mode])]

    def describe(self, mode, which, idx):
        """locate() with the plan the library gives this problem now (host arithmetic: works without a GPU)."""
        from mtl_ssl_amd import ops
        from mtl_ssl_amd.lib import ConvDesc
        d = ConvDesc(*self.prob, 0)
        return locate(self.prob, mode, which, idx, ops.conv_plan_info(d, mode), lambda c: ops.conv_plan_info(d, mode, c))

    def check_whole(self, mode, outs, bound, tag, note=None):
        """check_errors over EVERY element of the mode's outputs, against float64 references built on the operands'
        device (prepare_whole; pinned to the CPU reference on the sample first, the figures in whole_stats[mode]). A miss
        names the worst element — row, column, tile, split — lists the 20 worst, counts the elements beyond the bound and
        gives the error of a plain float32 tap walk of the same operands in the same unit. -> errs."""
        found = self.whole_errors(mode, outs)
        self.whole_stats[mode] = dict(elements=sum(o.numel() for o in _tuple(outs)), ref_diff=self.reference_difference(mode))
        errs = [e for e, _ in found]
        lims = [bound] + [DIRECT_BOUND] * (len(errs) - 1)
        if note is not None:
            note(errs, lims)
        if all(e <= lim for e, lim in zip(errs, lims)):
            return errs
        plain = self.prepare_whole(mode, torch.float32)
        lines = []
        for which, (o, (ref, mag), (e, at), lim) in enumerate(zip(_tuple(outs), self.whole[mode], found, lims)):
            if e <= lim:
                continue
            top, beyond = worst_whole(o, ref, mag, lim)
            lines.append("%s whole output %d: worst %.2f > %s at %s; %d of %d elements beyond; a plain float32 tap walk: %.2f" % (
                MODE_NAMES[mode], which, e, lim, self.describe(mode, which, at), beyond, o.numel(),
                dot_err_whole(plain[which][0], ref, mag)[0]))
            lines += ["    %.2f at %s" % (v, self.describe(mode, which, i)) for v, i in top]
        raise AssertionError("\n".join(lines + [repr(tag)]))

    def check_exact_epilogue(self, mode, got, linear, *ctx):
        """The nonlinear epilogues are exact functions of the linear result (the split-K fold sums in a fixed order)."""
        from mtl_ssl_amd import ops as O
        if mode == 0:
            assert torch.equal(got, apply_fwd_epilogue(linear, O.EPI_RELU)), ("forward ReLU epilogue",) + ctx
        if mode == 1:
            assert torch.equal(got, apply_dgrad_epilogue(linear, O.EPI_MASK, mask_ref=self.mask)), ("dgrad mask epilogue",) + ctx

