"""Float64 references and output samplers shared by the plan tests (test_gpu_plan_table.py, test_gpu_offtable_plans.py):
the reference never shortens a reduction, it samples outputs instead — flat output rows of the forward (all K channels
each) and input rows of the dgrad (all C channels), tile boundaries and image corners included, and every (r, s) tap of a
channel block of the filter gradient summed over all N*OH*OW pixels. Each returns (sum, sum |a*b|) for
tests/parity_report.py dot_err. A plain module: no fixtures, not a conftest."""
import numpy as np
import torch

ROWS = 256                      # sampled rows of a forward output / dgrad input
CH = 16                         # sampled channels per side of the filter-gradient block
DIRECT_BOUND, WINO_BOUND = 8.0, 400.0       # the constants of tests/test_gpu_split_engine.py


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
