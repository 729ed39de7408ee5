"""Float64 definitions of batch-statistics BatchNorm (slim.batch_norm in training mode, the fused kernel) and the error
bounds the device kernels of mtl_ssl_amd/csrc/batch_norm.hip are held to. numpy only; tests/batch_norm/
test_batchnorm_ref.py ties the definitions to torch.nn.functional.batch_norm(training=True) and autograd.

Definitions over x [n, C] (n rows of the per-GPU batch), per channel:
    mean = sum(x) / n                  var = sum((x - mean)^2) / n        (biased, from deviations)
    inv_std = 1 / sqrt(var + eps)      xhat = (x - mean) * inv_std
    y = act(gamma * xhat + beta)       gamma None: 1, beta None: 0; act None | 'relu' | 'relu6'
    moving_mean -= (moving_mean - mean) * f
    moving_var  -= (moving_var - var * n / max(n - 1, 1)) * f             f = float32(1 - float64(float32(decay)))
    g = dy * mask(y)    dbeta = sum(g)    dgamma = sum(g * xhat)
    dx = gamma * inv_std * (g - sum(g)/n - xhat * sum(g * xhat)/n)

Bounds, per rounding, in units of u = 2^-24 (fp32 round to nearest: |fl(a op b) - (a op b)| <= u |a op b|), first order
in u. The kernel's header states its reduction: each of 64 row lanes sums s(n) = ceil(n / 64) terms serially (s - 1
roundings: the first term is added to an exact zero), the lanes combine in a tree of depth d = 6 (d roundings on any
path). A sum S = sum(t_i) of exactly known terms therefore comes back with |error| <= (s - 1 + d) u sum|t_i|.

  mean      the sum, then one division:                                E_mean = (s + d) u sum|x| / n
  var       with the device's mean m' = mean + e, sum((x - m')^2)/n = var + e^2 exactly; each term carries three
            roundings (the difference, squared: 2 u; the product: u), the sum s - 1 + d, the division 1:
                                                                       E_var = (s + d + 3) u var + E_mean^2
            (the factor (1 + (s+d+3) u) on e^2 is dropped: it is second order)
  inv_std   1/sqrt is monotone in var, so its error over [var - E_var, var + E_var] (clipped at 0: the device's var is
            a sum of squares) is attained at an end; the addition of eps, the square root (which halves a relative
            error) and the division add at most 3 u relative:
                                   E_is = max|1/sqrt(var -+ E_var + eps) - inv_std| (1 + 3u) + 3 u inv_std
  y         a = |x - mean|. The device's x - m' is off by E_mean and one rounding; times inv_std' (off by E_is), one
            rounding; times gamma, one; plus beta, one on the result. With xh = (a + E_mean)(inv_std + E_is) >= |xhat'|:
                   E_y = |gamma| ((a + E_mean) E_is + inv_std E_mean) + 3 u |gamma| xh + u (|gamma| xh + |beta|)
            ReLU / ReLU6 are 1-Lipschitz: the bound holds after them.
  moving_*  not bounded: the device's update must EQUAL the unfused fp32 sequence on its own saved statistics.

The backward is checked with the device's save_mean / save_inv_std taken as given (exact inputs, in float64), so only
its own roundings count. xhat' = fl(fl(x - mean) inv_std): two roundings.
  dbeta     sum(g):                                                    E_db = (s + d) u sum|g|
  dgamma    sum(g xhat'): three roundings per term (two in xhat', the product), then the sum:
                                                                       E_dg = (s + d + 3) u sum|g xhat|
            (s + d, not s - 1 + d: one rounding of margin for the accumulate into an existing gradient, accum = 1,
            whose own rounding u |result| the callers add where they use it)
  dx        sg = fl(S_g / n): E_db / n + u |sg|; sgx likewise. p = fl(xhat' sgx): |xhat| E(sgx) + 3 u |p|.
            t1 = fl(g - sg), t = fl(t1 - p), k = fl(gamma inv_std), dx = fl(k t). With A = |g| + |sg| + |p|, which
            bounds |t1| and |t|, every rounding above is at most u A and there are eight of them:
                        E_dx = |k| (E_db / n + |xhat| E_dg / n + 8 u A)
"""
import math

import numpy as np

U = 2.0 ** -24
ROW_LANES = 64          # csrc/batch_norm.hip: BN_TY * BN_UNROLL
TREE_DEPTH = 6          # 2 levels in registers, 4 in LDS


def serial_run(n):
    """s(n) of the kernel's header comment."""
    return -(-int(n) // ROW_LANES)


def moving_average_factor(decay):
    return np.float32(1.0 - float(np.float32(decay)))


def _act(v, act):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "relu6":
        return np.minimum(np.maximum(v, 0.0), 6.0)
    assert act is None, act
    return v


def act_mask(y, act):
    if act == "relu":
        return y > 0
    if act == "relu6":
        return (y > 0) & (y < 6)
    assert act is None, act
    return np.ones(y.shape, bool)


def stats(x, eps):
    """-> mean, var (biased), inv_std, float64 [C]."""
    x = np.asarray(x, np.float64)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1.0 / np.sqrt(var + eps)


def forward(x, gamma, beta, eps, act=None):
    """-> y, mean, var, inv_std in float64."""
    x = np.asarray(x, np.float64)
    mean, var, inv_std = stats(x, eps)
    v = (x - mean) * inv_std
    if gamma is not None:
        v = v * np.asarray(gamma, np.float64)
    if beta is not None:
        v = v + np.asarray(beta, np.float64)
    return _act(v, act), mean, var, inv_std


def moving_update(moving_mean, moving_var, mean, var, n, f):
    """The float64 definition (the device's is checked against moving_update_fp32)."""
    mm, mv = np.asarray(moving_mean, np.float64), np.asarray(moving_var, np.float64)
    unbiased = np.asarray(var, np.float64) * n / max(n - 1, 1)
    return mm - (mm - mean) * float(f), mv - (mv - unbiased) * float(f)


def moving_update_fp32(moving, value, f):
    """moving - (moving - value) * f as one unfused fp32 sequence (assign_moving_average, zero_debias=False)."""
    moving, value, f = np.asarray(moving, np.float32), np.asarray(value, np.float32), np.float32(f)
    return (moving - ((moving - value) * f).astype(np.float32)).astype(np.float32)


def unbiased_fp32(var, n):
    """(var * n) / max(n - 1, 1) as the kernel's fp32 sequence."""
    var = np.asarray(var, np.float32)
    return ((var * np.float32(n)).astype(np.float32) / np.float32(max(n - 1, 1))).astype(np.float32)


def backward(x, dy, y, gamma, mean, inv_std, act=None):
    """-> dx, dgamma, dbeta, and (g, xhat) in float64, with mean / inv_std as given."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = x.shape[0]
    g = dy * act_mask(np.asarray(y), act) if act is not None else dy
    xhat = (x - np.asarray(mean, np.float64)) * np.asarray(inv_std, np.float64)
    sg, sgx = g.sum(0), (g * xhat).sum(0)
    k = np.asarray(inv_std, np.float64) * (1.0 if gamma is None else np.asarray(gamma, np.float64))
    dx = k * (g - sg / n - xhat * (sgx / n))
    return dx, sgx, sg, (g, xhat)


# ----------------------------------------------------------------------------------------------- bounds (docstring)
def forward_bounds(x, gamma, beta, eps):
    """-> dict of float64 bounds: mean, var, inv_std [C], y [n, C] (valid after any of the activations)."""
    x = np.asarray(x, np.float64)
    n, C = x.shape
    s, d = serial_run(n), TREE_DEPTH
    mean, var, inv_std = stats(x, eps)
    e_mean = (s + d) * U * np.abs(x).sum(0) / n
    e_var = (s + d + 3) * U * var + e_mean ** 2
    lo, hi = np.maximum(var - e_var, 0.0), var + e_var
    e_is = np.maximum(np.abs(1.0 / np.sqrt(lo + eps) - inv_std), np.abs(1.0 / np.sqrt(hi + eps) - inv_std)) \
        * (1 + 3 * U) + 3 * U * inv_std
    ga = np.ones(C) if gamma is None else np.abs(np.asarray(gamma, np.float64))
    be = np.zeros(C) if beta is None else np.abs(np.asarray(beta, np.float64))
    a = np.abs(x - mean)
    xh = (a + e_mean) * (inv_std + e_is)
    e_y = ga * ((a + e_mean) * e_is + inv_std * e_mean) + 3 * U * ga * xh + U * (ga * xh + be)
    return dict(mean=e_mean, var=e_var, inv_std=e_is, y=e_y)


def backward_bounds(x, dy, y, gamma, mean, inv_std, act=None):
    """-> dict of float64 bounds: dbeta, dgamma [C], dx [n, C], for save_mean / save_inv_std taken as given."""
    dx, sgx, sg, (g, xhat) = backward(x, dy, y, gamma, mean, inv_std, act)
    n = g.shape[0]
    s, d = serial_run(n), TREE_DEPTH
    e_db = (s + d) * U * np.abs(g).sum(0)
    e_dg = (s + d + 3) * U * np.abs(g * xhat).sum(0)
    k = np.abs(np.asarray(inv_std, np.float64) * (1.0 if gamma is None else np.asarray(gamma, np.float64)))
    A = np.abs(g) + np.abs(sg / n) + np.abs(xhat * (sgx / n))
    e_dx = k * (e_db / n + np.abs(xhat) * e_dg / n + 8 * U * A)
    return dict(dbeta=e_db, dgamma=e_dg, dx=e_dx)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements; an exact match where the bound is 0 counts as 0, a miss as inf."""
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def cases_input(n, C, seed):
    """fp32 test input [n, C]: unit normal columns; column 0 constant 3.0 (sums of up to 2^22 copies are exact, so
    var == 0 exactly), column C - 1 (when C > 1) = 1000 + 1e-3 * noise."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, C)).astype(np.float32)
    x[:, 0] = 3.0
    if C > 1:
        x[:, C - 1] = (1000.0 + 1e-3 * rng.standard_normal(n)).astype(np.float32)
    return x


assert math.isclose(U, np.finfo(np.float32).eps / 2)
