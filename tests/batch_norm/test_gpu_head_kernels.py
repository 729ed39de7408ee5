"""mtlssl_batch_norm_train_fwd / _bwd against the float64 definitions of batchnorm_ref.py on the same fp32 inputs, inside
the per-rounding bounds derived in that module's docstring (serial run s(rows) = ceil(rows / 64), tree depth d = 6, as
the kernel's header states). Every operand sits between guard bands (tests/footprint/guarded.py), outputs start as NaN,
and every call is made twice: the second result must equal the first bit for bit.

Inputs (batchnorm_ref.cases_input): column 0 is the constant 3.0 (var == 0 exactly, mean exact), the last column is
1000 + 1e-3 * noise, the others unit normal."""
import numpy as np
import pytest
import torch

from tests.batch_norm import batchnorm_ref as R
from tests.footprint import guarded as G

pytestmark = pytest.mark.gpu

EPS = 1e-3
# rows in {1, 2, 63, 64, 65, 257, 4864} x C in {1, 3, 21, 64, 84, 512, 1000}: every value of each, the extremes crossed
SHAPES = [(1, 1), (1, 1000), (2, 3), (63, 21), (64, 64), (65, 84), (257, 512), (257, 1000), (4864, 1), (4864, 21),
          (4864, 512), (4864, 1000)]
# (gamma, beta, activation, accum of the backward's parameter gradients)
VARIANTS = [(True, True, None, 0.0), (True, True, "relu", 1.0), (True, True, "relu6", 0.0), (False, True, "relu", 0.0),
            (True, False, None, 1.0), (False, False, None, 0.0)]
_ID = {None: "linear", "relu": "relu", "relu6": "relu6"}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("gamma_on,beta_on,act,accum", VARIANTS,
                         ids=["%s%s-%s-accum%d" % ("g" if g else "", "b" if b else "", _ID[a], c) for g, b, a, c in VARIANTS])
@pytest.mark.parametrize("rows,C", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_forward_and_backward_against_float64(ops, rows, C, gamma_on, beta_on, act, accum):
    rng = np.random.RandomState(rows * 1009 + C)
    x = R.cases_input(rows, C, rows + C)
    # gamma up to 4.5: with ReLU6 some outputs pass 6
    gamma = rng.uniform(0.5, 4.5, C).astype(np.float32) if gamma_on else None
    beta = rng.uniform(-0.5, 0.5, C).astype(np.float32) if beta_on else None
    dy = rng.standard_normal((rows, C)).astype(np.float32)
    mm0 = rng.uniform(-1, 1, C).astype(np.float32)
    mv0 = rng.uniform(0.5, 2, C).astype(np.float32)
    f = R.moving_average_factor(0.999)
    epi = {None: 0, "relu": ops.EPI_RELU, "relu6": ops.EPI_RELU6}[act]
    mask = {None: 0, "relu": ops.EPI_MASK, "relu6": ops.EPI_MASK6}[act]

    gs = G.GuardSet()
    d_x, d_gamma, d_beta = (gs.input(_dev(a), k) if a is not None else None for a, k in ((x, "x"), (gamma, "gamma"), (beta, "beta")))

    def fwd(tag, moving=True, factor=f, mv_start=mv0):
        y = gs.output((rows, C), "y " + tag)
        sm, si = gs.output((C,), "save_mean " + tag), gs.output((C,), "save_inv_std " + tag)
        mm = gs.output((C,), "moving_mean " + tag, fill=_dev(mm0)) if moving else None
        mv = gs.output((C,), "moving_var " + tag, fill=_dev(mv_start)) if moving else None
        ops.batch_norm_train_fwd(d_x, d_gamma, d_beta, EPS, epi, mm, mv, float(factor), y=y, save_mean=sm, save_inv_std=si)
        return y, sm, si, mm, mv

    first, second = fwd("1"), fwd("2")
    # the device's Bessel-corrected variance, read through an update from zero with f = 1: 0 - (0 - v) * 1 == v exactly
    probe = fwd("probe", factor=1.0, mv_start=np.zeros(C, np.float32))
    gs.check()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "two forward calls on the same data differ"
    y, sm, si, mm, mv = (t.cpu().numpy() for t in first)
    for name, t in (("y", y), ("save_mean", sm), ("save_inv_std", si), ("moving_mean", mm), ("moving_var", mv)):
        assert np.isfinite(t).all(), name

    ry, rmean, rvar, ris = R.forward(x, gamma, beta, EPS, act)
    b = R.forward_bounds(x, gamma, beta, EPS)
    ratios = {"mean": R.worst_ratio(sm, rmean, b["mean"]), "inv_std": R.worst_ratio(si, ris, b["inv_std"]),
              "y": R.worst_ratio(y, ry, b["y"])}
    # the variance itself leaves the kernel only Bessel-corrected: (var * n) / max(n - 1, 1), two more roundings
    bessel = rows / max(rows - 1, 1)
    unbiased = probe[4].cpu().numpy()
    ratios["var"] = R.worst_ratio(unbiased, rvar * bessel, b["var"] * bessel + 2 * R.U * rvar * bessel)
    assert sm[0] == 3.0 and unbiased[0] == 0.0, "the constant column: mean and variance are exact"

    # the moving update is the unfused fp32 sequence on the device's own statistics, exactly
    assert np.array_equal(mm, R.moving_update_fp32(mm0, sm, f))
    assert np.array_equal(mv, R.moving_update_fp32(mv0, unbiased, f))
    # without moving vectors the same y and statistics
    bare = fwd("bare", moving=False)
    assert all(torch.equal(a, c) for a, c in zip(first[:3], bare[:3]))

    # ---- backward: the device's y (the mask) and saved statistics taken as given
    old_g, old_b = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    d_dy = gs.input(_dev(dy), "dy")

    def bwd(tag):
        dxo = gs.output((rows, C), "dx " + tag)
        prefill = (lambda o: _dev(o)) if accum else (lambda o: float("nan"))
        dgo = gs.output((C,), "dgamma " + tag, fill=prefill(old_g)) if gamma_on else None
        dbo = gs.output((C,), "dbeta " + tag, fill=prefill(old_b)) if beta_on else None
        ops.batch_norm_train_bwd(d_x, d_dy, d_gamma, first[1], first[2], dgo, dbo, y=first[0] if mask else None,
                                 mask_epilogue=mask, accum=accum, dx=dxo)
        return dxo, dgo, dbo

    b1, b2 = bwd("1"), bwd("2")
    gs.check()
    for a, c in zip(b1, b2):
        assert (a is None and c is None) or torch.equal(a, c), "two backward calls on the same data differ"
    rdx, rdg, rdb, _ = R.backward(x, dy, y, gamma, sm, si, act)
    bb = R.backward_bounds(x, dy, y, gamma, sm, si, act)
    dxv = b1[0].cpu().numpy()
    assert np.isfinite(dxv).all()
    ratios["dx"] = R.worst_ratio(dxv, rdx, bb["dx"])
    for name, out, want, old in (("dgamma", b1[1], rdg, old_g), ("dbeta", b1[2], rdb, old_b)):
        if out is None:
            continue
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), name
        want = want + (accum * old.astype(np.float64) if accum else 0.0)
        # accumulating adds one rounding of the result
        ratios[name] = R.worst_ratio(got, want, bb[name] + (R.U * np.abs(want) if accum else 0.0))
    line = "batch_norm %dx%d %s%s %s: worst error / bound " % (rows, C, "g" if gamma_on else "-", "b" if beta_on else "-",
                                                               _ID[act])
    line += ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))
    print(line)
    for name, r in ratios.items():
        assert r <= 1.0, (name, r)


def test_bad_arguments_are_refused(ops):
    from mtl_ssl_amd.lib import MtlsslError
    x = torch.zeros((4, 8), device="cuda")
    with pytest.raises(MtlsslError):
        ops.batch_norm_train_fwd(x, None, None, EPS, ops.EPI_TANH)
    with pytest.raises(MtlsslError):          # a mask needs y
        ops.batch_norm_train_bwd(x, x.clone(), None, torch.zeros(8, device="cuda"), torch.ones(8, device="cuda"), None,
                                 None, y=None, mask_epilogue=ops.EPI_MASK)
