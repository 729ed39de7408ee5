"""CPU: the float64 references of tests/spatial_ref.py against their fp32 torch counterparts in oracle/ops_torch.py
(autograd for the gradients) on small random cases, and the float32 coordinate restatement against the oracle's on
boxes that land exactly on integers, on H-1, on 0 and just outside. Keeps the references honest and independent of the
kernels they judge. Agreement is to fp32 rounding of the ORACLE: a few eps of the operands' magnitude per element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

from oracle import ops_torch as T
from tests import spatial_ref as S

EPS = float(np.finfo(np.float32).eps)
f32 = np.float32


def close(ref64, got32, mag, ulps, what):
    err = np.abs(np.asarray(got32, np.float64) - ref64)
    tol = ulps * EPS * np.asarray(mag, np.float64)
    bad = ~(err <= tol)
    assert not bad.any(), "%s: %d elements differ, worst %r vs %r" % (
        what, int(bad.sum()), float(err.max()), float(np.broadcast_to(tol, err.shape)[np.unravel_index(err.argmax(), err.shape)]))


def edge_boxes():
    """Boxes whose samples land on 0, on n-1, on interior integers and one float32 step outside the map."""
    up, dn = np.nextafter(f32(1), f32(2)), np.nextafter(f32(0), f32(-1))
    b = [[0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 0, 0], [0.5, 0.5, 0.5, 0.5], [0, 0, up, up], [dn, dn, 1, 1],
         [up, up, up, up], [dn, dn, dn, dn], [-0.2, 0.3, 0.4, 1.3], [0.25, 0.75, 0.75, 0.25], [0.3, 0.3, 0.3001, 0.3001]]
    return np.array(b, f32)


@pytest.mark.parametrize("H,W,crop", [(9, 13, 5), (38, 64, 14), (7, 7, 1), (50, 84, 17), (5, 9, 9)])
def test_crop_coordinates_agree_with_the_oracle_on_edge_boxes(H, W, crop):
    rs = np.random.RandomState(H * W)
    boxes = np.concatenate([edge_boxes(), (rs.rand(20, 4) * 1.3 - 0.15).astype(f32)])
    for col, n in ((0, H), (1, W)):
        pos, valid, i0, i1, frac = S.crop_axis(boxes[:, col], boxes[:, col + 2], n, crop)
        lo, hi = torch.from_numpy(boxes[:, col:col + 1]), torch.from_numpy(boxes[:, col + 2:col + 3])
        if crop > 1:                                              # oracle/ops_torch.py crop_and_resize, verbatim
            ref = lo * (n - 1) + torch.arange(crop, dtype=torch.float32)[None, :] * ((hi - lo) * (n - 1) / (crop - 1))
        else:
            ref = 0.5 * (lo + hi) * (n - 1)
        np.testing.assert_array_equal(pos.view(np.int32), ref.numpy().view(np.int32))
        rv = (ref >= 0) & (ref <= n - 1)
        np.testing.assert_array_equal(valid, rv.numpy())
        np.testing.assert_array_equal(i0[valid], torch.floor(ref).long().numpy()[valid])
        np.testing.assert_array_equal(i1[valid], torch.ceil(ref).long().numpy()[valid])
        np.testing.assert_array_equal(frac.view(np.int32), (ref - torch.floor(ref)).numpy().view(np.int32))
    # the cases the set exists for are present: a sample exactly on n-1, one exactly on 0, one just outside each end
    pos, valid, *_ = S.crop_axis(boxes[:, 0], boxes[:, 2], H, crop)
    assert (pos[valid] == H - 1).any() and (pos[valid] == 0).any()
    assert (~valid & (pos > H - 1) & (pos < H)).any() and (~valid & (pos < 0) & (pos > -1)).any()


@pytest.mark.parametrize("crop,pk,ps", [(6, 2, 2), (5, 1, 1), (1, 1, 1), (7, 3, 2)])
def test_crop_and_resize_and_its_gradient_against_the_oracle(crop, pk, ps):
    rs = np.random.RandomState(crop)
    feat = rs.randn(2, 9, 13, 4).astype(f32)
    boxes = np.concatenate([edge_boxes(), (rs.rand(15, 4) * 1.2 - 0.1).astype(f32)])
    bi = rs.randint(0, 2, len(boxes))
    val, amax, valid = S.crop_and_resize(feat, boxes, bi, crop)
    fr = torch.from_numpy(feat).requires_grad_()
    ref = T.crop_and_resize(fr, torch.from_numpy(boxes), torch.from_numpy(bi), crop)
    close(val, ref.detach().numpy(), amax, 5, "crop_and_resize")           # three lerps of three roundings: see the GPU test
    assert (val[~valid] == 0).all() and (ref.detach().numpy()[~valid] == 0).all()
    win = S.pool_windows(val, pk, ps)
    sel = win.argmax(3)                                                        # first maximum in window order
    pooled = T.max_pool(ref, pk, ps, "VALID") if pk > 1 else ref
    close(win.max(3), pooled.detach().numpy(), S.pool_windows(amax, pk, ps).max(3), 5, "pooled crops")
    gy = rs.randn(*pooled.shape).astype(f32)
    pooled.backward(torch.from_numpy(gy))
    # the oracle's arg-max is its own (fp32); compare only where the float64 maximum is clear of the runner-up
    srt = np.sort(win, 3)
    clear = (pk == 1) | ((srt[:, :, :, -1] - srt[:, :, :, -2 if pk > 1 else -1]) > 10 * EPS * S.pool_windows(amax, pk, ps).max(3))
    grad, n, sabs = S.roi_crop_pool_bwd(np.where(clear, gy, 0).astype(f32), sel, feat.shape, boxes, bi, crop, pk, ps)
    fr2 = torch.from_numpy(feat).requires_grad_()
    r2 = T.crop_and_resize(fr2, torch.from_numpy(boxes), torch.from_numpy(bi), crop)
    (T.max_pool(r2, pk, ps, "VALID") if pk > 1 else r2).backward(torch.from_numpy(np.where(clear, gy, 0).astype(f32)))
    # autograd differentiates tl + (tr - tl) * xl as g - g * xl: its rounding is relative to |g|, not to |g * weight|
    close(grad, fr2.grad.numpy(), sabs + n * np.abs(gy).max(), 8 + n.max(), "crop_and_resize gradient")
    assert (grad[n == 0] == 0).all() and (fr2.grad.numpy()[n == 0] == 0).all()


def test_psroi_and_its_gradient_against_the_oracle():
    rs = np.random.RandomState(3)
    bins, crop, Cc = (3, 3), (6, 6), 5
    fmap = rs.randn(2, 9, 13, 9 * Cc).astype(f32)
    boxes = np.concatenate([edge_boxes(), (rs.rand(15, 4) * 1.2 - 0.1).astype(f32)])
    bi = rs.randint(0, 2, len(boxes))
    val, sumA = S.psroi(fmap, boxes, bi, crop, bins)
    fr = torch.from_numpy(fmap).requires_grad_()
    ref = T.position_sensitive_crop_regions(fr, torch.from_numpy(boxes), torch.from_numpy(bi), crop, bins, True)[:, 0, 0]
    close(val, ref.detach().numpy(), sumA, 5 + 36 + 9, "psroi")
    gy = rs.randn(*ref.shape).astype(f32)
    ref.backward(torch.from_numpy(gy))
    grad, n, sabs = S.psroi_bwd(gy, fmap.shape, boxes, bi, crop, bins)
    # as above, autograd's g - g * xl rounds relative to |g|: every RoI of the image may leave eps * |g| / 36 behind
    close(grad, fr.grad.numpy(), sabs + len(boxes) * np.abs(gy).max() / 36, 40 + n.max(), "psroi gradient")
    assert (grad[n == 0] == 0).all()


@pytest.mark.parametrize("H,W,OH,OW", [(5, 9, 8, 8), (12, 7, 8, 8), (8, 8, 8, 8), (1, 1, 4, 4), (16, 16, 8, 8)])
def test_resize_and_its_gradient_against_the_oracle(H, W, OH, OW):
    rs = np.random.RandomState(H + W)
    x = rs.randn(2, H, W, 3).astype(f32)
    val, amax = S.resize_bilinear(x, OH, OW)
    xr = torch.from_numpy(x).requires_grad_()
    ref = T.resize_bilinear_legacy(xr, OH, OW)
    close(val, ref.detach().numpy(), amax, 5, "resize")
    gy = rs.randn(*ref.shape).astype(f32)
    ref.backward(torch.from_numpy(gy))
    grad, n, sabs = S.resize_bilinear_bwd(gy, x.shape)
    close(grad, xr.grad.numpy(), sabs, 8 + n.max(), "resize gradient")
    # adjoint identity of the reference itself, in float64
    assert abs((val * gy).sum() - (x.astype(np.float64) * grad).sum()) <= 1e-12 * np.abs(val * gy).sum()


@pytest.mark.parametrize("k,stride,padding,shape", [(3, 2, "SAME", (2, 9, 12, 4)), (3, 2, "VALID", (1, 17, 17, 4)),
                                                     (2, 2, "VALID", (2, 8, 6, 4)), (1, 2, "SAME", (1, 7, 7, 4))])
def test_max_pool_and_its_gradient_against_the_oracle(k, stride, padding, shape):
    rs = np.random.RandomState(k)
    x = rs.randn(*shape).astype(f32)
    xr = torch.from_numpy(x).requires_grad_()
    ref = T.max_pool(xr, k, stride, padding)
    y = S.max_pool(x, k, stride, padding)
    np.testing.assert_array_equal(y, ref.detach().numpy())
    gy = rs.randn(*ref.shape).astype(f32)
    ref.backward(torch.from_numpy(gy))
    grad, n, sabs = S.max_pool_bwd(x, gy, k, stride, padding)
    close(grad, xr.grad.numpy(), sabs, n.max(), "max-pool gradient")
    assert n.sum() == gy.size                                                   # every window's gradient lands once


@pytest.mark.parametrize("padding", ["SAME", "VALID"])
@pytest.mark.parametrize("k,stride,shape", [(3, 1, (2, 9, 12, 4)), (2, 2, (1, 7, 8, 4)), (5, 2, (1, 11, 10, 4)), (3, 2, (1, 8, 7, 4))])
def test_avg_pool_and_its_gradient_against_torch(k, stride, shape, padding):
    rs = np.random.RandomState(k)
    x = rs.randn(*shape).astype(f32)
    xr = torch.from_numpy(x).requires_grad_()
    if padding == "SAME":
        ref = T.avg_pool_same(xr, k, stride)
    else:                                                                       # every window in bounds: a plain mean
        ref = Fnn.avg_pool2d(xr.permute(0, 3, 1, 2), k, stride).permute(0, 2, 3, 1)
    val, cnt, sabs = S.avg_pool(x, k, stride, padding)
    assert val.shape == tuple(ref.shape)
    close(val, ref.detach().numpy(), sabs / cnt[None, :, :, None], k * k + 1, "avg-pool")
    gy = rs.randn(*ref.shape).astype(f32)
    ref.backward(torch.from_numpy(gy))
    grad, n, sg = S.avg_pool_bwd(gy, x.shape, k, stride, padding)
    close(grad, xr.grad.numpy(), sg, k * k + 1, "avg-pool gradient")


@pytest.mark.parametrize("stride,dilation,shape", [(1, 1, (2, 9, 12, 8)), (2, 1, (1, 9, 12, 8)), (2, 1, (1, 8, 7, 4)), (1, 2, (1, 9, 9, 4))])
def test_depthwise_and_its_gradients_against_the_oracle(stride, dilation, shape):
    rs = np.random.RandomState(stride)
    x = rs.randn(*shape).astype(f32)
    w = rs.randn(3, 3, shape[3]).astype(f32)
    xr, wr = torch.from_numpy(x).requires_grad_(), torch.from_numpy(w[..., None]).requires_grad_()
    ref = T.depthwise_conv2d(xr, wr, stride, dilation)
    val, sabs = S.depthwise(x, w, stride, dilation)
    close(val, ref.detach().numpy(), sabs, 10, "depthwise")
    g = rs.randn(*ref.shape).astype(f32)
    ref.backward(torch.from_numpy(g))
    dx, sx = S.depthwise_dgrad(g, w, x.shape, stride, dilation)
    close(dx, xr.grad.numpy(), sx, 10, "depthwise dgrad")
    dw, sw = S.depthwise_wgrad(x, g, stride, dilation)
    close(dw, wr.grad.numpy()[..., 0], sw, g.size // shape[3], "depthwise wgrad")


def test_bn_param_grads_against_autograd():
    rs = np.random.RandomState(0)
    rows, C = 37, 8
    gamma = rs.randn(C).astype(f32)
    gamma[3] = 0.0
    beta = rs.randn(C).astype(f32)
    xhat = rs.randn(rows, C).astype(f32)
    gm, bt = torch.from_numpy(gamma).requires_grad_(), torch.from_numpy(beta).requires_grad_()
    y = gm * torch.from_numpy(xhat) + bt
    g = rs.randn(rows, C).astype(f32)
    y.backward(torch.from_numpy(g))
    dgamma, dbeta, s_gy, s_g = S.bn_param_grads(y.detach().numpy(), g, gamma, beta)
    close(dbeta, bt.grad.numpy(), s_g, rows, "dbeta")
    nz = gamma != 0
    # y - beta recovers gamma * xhat to one rounding of y: eps * |y| per term, amplified by 1 / gamma
    ymag = (np.abs(g) * np.abs(y.detach().numpy())).sum(0)
    close(dgamma[nz], gm.grad.numpy()[nz], (s_gy + ymag)[nz] / np.abs(gamma[nz]), rows, "dgamma")
    assert dgamma[3] == 0.0


def test_spatial_mean_against_torch():
    rs = np.random.RandomState(1)
    x = rs.randn(3, 5, 7, 6).astype(f32)
    m, sabs = S.spatial_mean(x)
    close(m, torch.from_numpy(x).mean((1, 2)).numpy(), sabs / 35, 36, "spatial mean")
    act = rs.randn(3, 5, 7, 6).astype(f32) * 4
    act[0, 0, 0, :3] = (0.0, 6.0, 3.0)
    dy = rs.randn(3, 6).astype(f32)
    for relu6 in (False, True):
        ar = torch.from_numpy(act).requires_grad_()
        (Fnn.relu6(ar) if relu6 else torch.relu(ar)).mean((1, 2)).backward(torch.from_numpy(dy))
        # torch's relu6 (hardtanh) passes the gradient AT 6, TF's does not (relu6 grad: 0 < x < 6): skip those
        keep = act != 6
        ref = S.spatial_mean_bwd(dy, act.shape, act, relu6)
        close(ref[keep], ar.grad.numpy()[keep], np.abs(ref[keep]), 2, "masked mean gradient")
        assert ref[0, 0, 0, 0] == 0 and ref[0, 0, 0, 2] != 0 and (ref[0, 0, 0, 1] == 0) == relu6


def test_expand_windows_and_clip():
    rs = np.random.RandomState(2)
    p = np.sort(rs.rand(2, 11, 2, 2).astype(f32), 2).reshape(2, 11, 4)
    w32, w64 = S.expand_windows_f32(p, 5), S.expand_windows(p, 5)
    np.testing.assert_array_equal(w32[:, 0], p)
    close(w64, w32, 1.0, 2, "expand_windows")                      # coordinates and offsets are all <= 1
    np.testing.assert_allclose(w64[:, -1], np.broadcast_to([0, 0, 1, 1], p.shape), atol=1e-15)
    b = (rs.rand(9, 4) * 3 - 1).astype(f32)
    c = S.clip_to_window(b, (0.0, 0.25, 1.0, 0.75))
    np.testing.assert_array_equal(c, torch.from_numpy(b).clamp(
        torch.tensor([0, 0.25, 0, 0.25]), torch.tensor([1, 0.75, 1, 0.75])).numpy())


def test_recorded_depthwise_layer_list_matches_the_model():
    """The depthwise shapes the GPU file records are the ones mobilenet.py builds, and its restated reduce_plan reaches
    the branch the extra shapes are there for (no GPU needed: the GPU file only carries the mark)."""
    from tests import test_gpu_spatial_kernels as G
    assert sorted(set(G.mobilenet_depthwise_layers())) == sorted(set(G.DW_LAYERS))
    assert G.reduce_plan(513, 36)[1:4] == (16, 17, 32) and 513 % 32 == 1
