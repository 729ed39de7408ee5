"""CPU twin of batchnorm_ref.py: its float64 definitions are torch.nn.functional.batch_norm(training=True) and its
autograd, and its bounds reject each wrong variant of the semantics that a kernel could compute
instead."""
import numpy as np
import pytest
import torch

from tests.batch_norm import batchnorm_ref as R

EPS = 1e-3


def _data(n, C, seed=0):
    rng = np.random.RandomState(seed)
    x = R.cases_input(n, C, seed)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, C).astype(np.float32)
    dy = rng.standard_normal((n, C)).astype(np.float32)
    return x, gamma, beta, dy


@pytest.mark.parametrize("n,C", [(2, 3), (65, 21), (257, 64)])
@pytest.mark.parametrize("affine", ["gamma_beta", "beta", "none"])
def test_definitions_are_torch_batch_norm_in_float64(n, C, affine):
    x, gamma, beta, dy = _data(n, C)
    gamma = gamma if affine == "gamma_beta" else None
    beta = beta if affine != "none" else None
    f = R.moving_average_factor(0.999)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tg = None if gamma is None else torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    tb = None if beta is None else torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    rm, rv = torch.full((C,), 0.25, dtype=torch.float64), torch.full((C,), 2.0, dtype=torch.float64)
    ty = torch.nn.functional.batch_norm(tx, rm, rv, tg, tb, training=True, momentum=float(f), eps=EPS)
    ty.backward(torch.tensor(dy, dtype=torch.float64))
    y, mean, var, inv_std = R.forward(x, gamma, beta, EPS)
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-10, atol=1e-9)
    mm, mv = R.moving_update(np.full(C, 0.25), np.full(C, 2.0), mean, var, n, f)
    np.testing.assert_allclose(mm, rm.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(mv, rv.numpy(), rtol=1e-12, atol=1e-12)          # Bessel-corrected
    dx, dgamma, dbeta, _ = R.backward(x, dy, y, gamma, mean, inv_std)
    np.testing.assert_allclose(dx, tx.grad.numpy(), rtol=1e-8, atol=1e-8)
    if tg is not None:
        np.testing.assert_allclose(dgamma, tg.grad.numpy(), rtol=1e-9, atol=1e-9)
    if tb is not None:
        np.testing.assert_allclose(dbeta, tb.grad.numpy(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("act", ["relu", "relu6"])
def test_activation_mask_is_autograd_of_the_activation(act):
    x, gamma, beta, dy = _data(65, 21, 1)
    gamma = gamma * 4.0                      # some outputs beyond 6
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor(gamma, dtype=torch.float64, requires_grad=True)
    tb = torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    pre = torch.nn.functional.batch_norm(tx, None, None, tg, tb, training=True, eps=EPS)
    ty = torch.relu(pre) if act == "relu" else torch.clamp(pre, 0.0, 6.0)
    ty.backward(torch.tensor(dy, dtype=torch.float64))
    y, mean, var, inv_std = R.forward(x, gamma, beta, EPS, act)
    np.testing.assert_allclose(y, ty.detach().numpy(), rtol=1e-10, atol=1e-9)
    dx, dgamma, dbeta, _ = R.backward(x, dy, y, gamma, mean, inv_std, act)
    np.testing.assert_allclose(dx, tx.grad.numpy(), rtol=1e-8, atol=1e-8)
    np.testing.assert_allclose(dgamma, tg.grad.numpy(), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(dbeta, tb.grad.numpy(), rtol=1e-9, atol=1e-9)


def _fp32_forward(x, gamma, beta, eps):
    """The definitions evaluated in fp32 by numpy (pairwise sums: fewer roundings than the kernel's bound allows)."""
    n = np.float32(x.shape[0])
    mean = (x.sum(0, dtype=np.float32) / n).astype(np.float32)
    dv = (x - mean).astype(np.float32)
    var = ((dv * dv).sum(0, dtype=np.float32) / n).astype(np.float32)
    inv_std = (np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)).astype(np.float32)
    return ((dv * inv_std) * gamma + beta).astype(np.float32), mean, var, inv_std


def test_an_honest_fp32_evaluation_is_inside_the_bounds():
    x, gamma, beta, dy = _data(257, 64)
    y, mean, var, inv_std = _fp32_forward(x, gamma, beta, EPS)
    ry, rmean, rvar, ris = R.forward(x, gamma, beta, EPS)
    b = R.forward_bounds(x, gamma, beta, EPS)
    for name, got, want in (("mean", mean, rmean), ("var", var, rvar), ("inv_std", inv_std, ris), ("y", y, ry)):
        assert R.worst_ratio(got, want, b[name]) <= 1.0, name
    assert var[0] == 0.0 and mean[0] == 3.0                       # the constant column: exactly
    g = dy.astype(np.float64)
    xhat32 = ((x - mean).astype(np.float32) * inv_std).astype(np.float32)
    sg, sgx = dy.sum(0, dtype=np.float32), (dy * xhat32).sum(0, dtype=np.float32)
    k = (gamma * inv_std).astype(np.float32)
    dx32 = (k * ((dy - sg / np.float32(257)) - xhat32 * (sgx / np.float32(257)))).astype(np.float32)
    dx, dgamma, dbeta, _ = R.backward(x, g, None, gamma, mean, inv_std)
    bb = R.backward_bounds(x, g, None, gamma, mean, inv_std)
    assert R.worst_ratio(dx32, dx, bb["dx"]) <= 1.0
    assert R.worst_ratio(sgx, dgamma, bb["dgamma"]) <= 1.0 and R.worst_ratio(sg, dbeta, bb["dbeta"]) <= 1.0


# ----------------------------------------------------------------------------------------------- the wrong variants
def test_unbiased_variance_inside_the_normaliser_is_rejected():
    x, gamma, beta, _ = _data(65, 21)
    n = x.shape[0]
    y, mean, var, inv_std = R.forward(x, gamma, beta, EPS)
    wrong = (x - mean) / np.sqrt(var * n / (n - 1) + EPS) * gamma + beta
    b = R.forward_bounds(x, gamma, beta, EPS)
    assert R.worst_ratio(wrong, y, b["y"]) > 1.0
    assert R.worst_ratio(1.0 / np.sqrt(var * n / (n - 1) + EPS), inv_std, b["inv_std"]) > 1.0


def test_biased_variance_in_the_moving_update_is_rejected():
    x, _, _, _ = _data(65, 21)
    n = x.shape[0]
    _, mean, var, _ = _fp32_forward(x, np.float32(1), np.float32(0), EPS)
    f = R.moving_average_factor(0.999)
    mv = np.ones(21, np.float32)
    right = R.moving_update_fp32(mv, R.unbiased_fp32(var, n), f)
    wrong = R.moving_update_fp32(mv, var, f)
    assert not np.array_equal(right, wrong)
    # and the right one is the float64 definition to fp32 rounding: three roundings of values near one
    want = R.moving_update(np.zeros(21), mv, mean, var, n, f)[1]
    assert np.abs(right - want).max() <= 4 * R.U * np.abs(want).max()
    assert np.abs(wrong - want).max() > 4 * R.U * np.abs(want).max()


def test_e_x2_minus_mean2_is_rejected_on_the_offset_column():
    n, C = 257, 3
    x = R.cases_input(n, C, 0)
    col = x[:, C - 1]
    nn_ = np.float32(n)
    m = (col.sum(dtype=np.float32) / nn_).astype(np.float32)
    wrong = np.float32((col * col).sum(dtype=np.float32) / nn_ - m * m)
    _, var, _ = R.stats(x, EPS)
    b = R.forward_bounds(x, None, None, EPS)
    assert abs(float(wrong) - var[C - 1]) > b["var"][C - 1]
    # whatever the cancellation leaves — even an exact zero — is outside: the bound is below the variance itself
    assert b["var"][C - 1] < var[C - 1]
    _, _, var32, _ = _fp32_forward(x, np.float32(1), np.float32(0), EPS)
    assert abs(float(var32[C - 1]) - var[C - 1]) <= b["var"][C - 1]


def test_dx_without_the_sum_g_term_is_rejected():
    x, gamma, beta, dy = _data(65, 21)
    y, mean, var, inv_std = R.forward(x, gamma, beta, EPS)
    dx, dgamma, dbeta, (g, xhat) = R.backward(x, dy, y, gamma, mean, inv_std)
    wrong = gamma * inv_std * (g - xhat * dgamma / 65)
    assert R.worst_ratio(wrong, dx, R.backward_bounds(x, dy, y, gamma, mean, inv_std)["dx"]) > 1.0


def test_epsilon_outside_the_square_root_is_rejected():
    x, gamma, beta, _ = _data(65, 21)
    _, var, inv_std = R.stats(x, EPS)
    b = R.forward_bounds(x, gamma, beta, EPS)
    assert R.worst_ratio(1.0 / (np.sqrt(var[1:]) + EPS), inv_std[1:], b["inv_std"][1:]) > 1.0


def test_bessel_factor_at_one_row():
    var = np.zeros(3, np.float32)
    assert np.array_equal(R.unbiased_fp32(var, 1), var)                 # n / max(n - 1, 1) = 1
    with np.errstate(divide="ignore", invalid="ignore"):
        naive = var * np.float32(1) / np.float32(0)
    assert not np.isfinite(naive).any()
    x = R.cases_input(1, 3, 0)
    _, mean, v, _ = R.forward(x, None, None, EPS)
    mm, mv = R.moving_update(np.zeros(3), np.ones(3), mean, v, 1, R.moving_average_factor(0.999))
    assert np.isfinite(mv).all() and np.all(mv < 1.0)
