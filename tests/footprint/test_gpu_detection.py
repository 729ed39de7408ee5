"""Footprint of the size queries outside the convolution family: each ops.* wrapper is called once with the ordinary
workspace cache and once under GuardedWorkspaces / GuardedOutputs (tests/footprint/guarded.py) with guarded inputs,
at the edge sizes the oracle tests of tests/test_gpu_detection.py, test_gpu_postprocess.py, test_gpu_conv_ops.py,
tests/geometric and tests/summaries already hold to the oracle or to float64. Asserted: every guard intact, outputs
written in full where the contract says so (no 0xFF prefill left), results bit-identical between the two calls.

The module shares its name with tests/test_gpu_detection.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these kernel-level cases run in its first stage."""
import numpy as np
import pytest
import torch

from tests import parity_report
from tests.footprint.guarded import GuardedOutputs, GuardedWorkspaces, GuardSet
from tests.test_gpu_detection import _assign_case, cu, rand_boxes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), what


def _written(t, what):
    """No element of a fully written output still holds the 0xFF prefill of GuardedOutputs."""
    item = t.element_size()
    left = (_bits(t).view(-1, item) == 255).all(1)
    assert not bool(left.any()), "%s: %d elements were never written" % (what, int(left.sum()))


def _guarded_call(call, tensors):
    """call(**tensors) with the ordinary cache, then with guarded inputs, workspaces and wrapper-made outputs."""
    ref = call(**tensors)
    gs = GuardSet()
    gin = {k: (gs.input(v, k) if isinstance(v, torch.Tensor) else v) for k, v in tensors.items()}
    with GuardedWorkspaces() as gw, GuardedOutputs() as go:
        got = call(**gin)
    gw.check()
    go.check()
    gs.check()
    assert gw.handouts or go.tensors
    return ref, got, gw, go


def _note(what, gw):
    parity_report.add("footprint %s: %s" % (what, gw.report()))


@pytest.mark.parametrize("n", [50, 1000])
def test_rpn_proposals(ops, n):
    rng = np.random.RandomState(n)
    anchors = rand_boxes(rng, n, 600, 1024, 8.0)
    enc = (rng.randn(2, n, 4) * 0.5).astype(np.float32)
    logit = (rng.randn(2, n, 2) * 2).astype(np.float32)
    call = lambda enc, logit, anchors: ops.rpn_proposals(enc, logit, anchors, 600, 1024, 0.0, 0.7, 300)
    ref, got, gw, _ = _guarded_call(call, dict(enc=cu(enc), logit=cu(logit), anchors=cu(anchors)))
    assert gw.bytes_of("nms") == [ops.lib().rpn_proposals_workspace_bytes(2, n)]
    for a, b, what in zip(ref, got, ("boxes", "scores", "num")):
        _written(b, "rpn_proposals " + what)                  # zero padded behind num
        _same(a, b, "rpn_proposals " + what)
    _note("rpn_proposals B=2 n=%d" % n, gw)


@pytest.mark.parametrize("n,max_out", [(1, 5), (63, 10), (64, 64), (65, 300), (1000, 300)])
def test_nms(ops, n, max_out):
    rng = np.random.RandomState(n)
    bx = rand_boxes(rng, n, 600, 1024, 8.0)
    sc = rng.permutation(n).astype(np.float32) / n
    call = lambda boxes, scores: ops.nms(boxes, scores, 0.7, max_out)
    (sel0, num0), (sel, num), gw, _ = _guarded_call(call, dict(boxes=cu(bx), scores=cu(sc)))
    assert gw.bytes_of("nms") == [ops.lib().nms_workspace_bytes(n)]
    k = int(num0.item())
    assert int(num.item()) == k and k <= min(n, max_out)
    _same(sel0[:k], sel[:k], "nms selection")                 # the contract writes the first num entries only
    _note("nms n=%d" % n, gw)


@pytest.mark.parametrize("B,n,C,q_per_class,mpc,T", [(2, 300, 20, True, 100, 300), (2, 64, 5, False, 10, 20)])
def test_batch_multiclass_nms(ops, B, n, C, q_per_class, mpc, T):
    rng = np.random.RandomState(B * 1000 + n + C)
    q = C if q_per_class else 1
    H, W = 600.0, 1024.0
    cy, cx = rng.uniform(-30, H + 30, (B, n, q)), rng.uniform(-30, W + 30, (B, n, q))
    h, w = rng.uniform(5, 300, (B, n, q)), rng.uniform(5, 300, (B, n, q))
    boxes = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], -1).astype(np.float32)
    scores = rng.uniform(0, 1, (B, n, C)).astype(np.float32) ** 3
    nv = rng.randint(n // 2, n + 1, B).astype(np.int32)
    call = lambda boxes, scores, nv: ops.batch_multiclass_nms(boxes, scores, 0.05, 0.6, mpc, T, [0, 0, H, W], True, nv)
    ref, got, gw, _ = _guarded_call(call, dict(boxes=cu(boxes), scores=cu(scores), nv=cu(nv)))
    assert gw.bytes_of("mcnms") == [ops.lib().batch_multiclass_nms_workspace_bytes(B, n, C, mpc)]
    for a, b, what in zip(ref, got, ("boxes", "scores", "classes", "num")):
        _written(b, "batch_multiclass_nms " + what)
        _same(a, b, "batch_multiclass_nms " + what)
    _note("batch_multiclass_nms B=%d n=%d C=%d" % (B, n, C), gw)


@pytest.mark.parametrize("n,G", [(257, 0), (64, 1), (300, 5)])
def test_assign_targets(ops, n, G):
    rng = np.random.RandomState(100 + n + G)
    anchors, gts, ngt = _assign_case(rng, n, G)
    call = lambda anchors, gts, ngt, um: ops.assign_targets(anchors, gts, ngt, None, um, 0.7, 0.3, True)
    ref, got, gw, _ = _guarded_call(call, dict(anchors=cu(anchors), gts=cu(gts), ngt=cu(ngt), um=cu(np.zeros((1,), np.float32))))
    assert gw.bytes_of("assign") == [ops.lib().assign_targets_workspace_bytes(2, n, gts.shape[1])]
    assert set(ref) == set(got)
    for k in ref:
        if k != "match":                                      # (an unmatched anchor's match is -1: all 0xFF bytes by right)
            _written(got[k], "assign_targets " + k)
        _same(ref[k], got[k], "assign_targets " + k)
    _note("assign_targets B=2 n=%d G=%d" % (n, G), gw)


@pytest.mark.parametrize("algo,C", [(1, 32), (2, 24)], ids=["lds", "atomics"])
def test_roi_crop_pool_bwd(ops, algo, C):
    """Both routes behind mtlssl_roi_crop_pool_bwd_ex (the LDS one needs C % 16 == 0), B = 2, pooled crops. The LDS route
    is deterministic: bit-identical. The atomic route adds in arrival order: its guarded run is held to the LDS route's
    tolerance of tests/test_gpu_conv_ops.py (1e-5 relative) against the ordinary call."""
    g = torch.Generator().manual_seed(C)
    feat_shape, R, crop, pk = (2, 9, 11, C), 33, 6, 2
    yx = torch.rand(R, 2, generator=g) * 0.9 - 0.05
    hw = torch.rand(R, 2, generator=g) * 0.6 + 0.02
    boxes = torch.cat([yx, yx + hw], 1).cuda()
    bi = (torch.arange(R) % 2).int().cuda()
    feat = torch.randn(feat_shape, generator=g).cuda()
    out, am = ops.roi_crop_pool_fwd(feat, boxes, bi, crop, pk, pk)
    gy = torch.randn(out.shape, generator=g).cuda()
    call = lambda gy, am, boxes, bi: ops.roi_crop_pool_bwd(gy, am, feat_shape, boxes, bi, crop, pk, pk, algo=algo)
    ref, got, gw, go = _guarded_call(call, dict(gy=gy, am=am, boxes=boxes, bi=bi))
    assert gw.bytes_of("roi_bwd") == [ops.lib().roi_crop_pool_bwd_workspace_bytes()]
    assert [tuple(t.shape) for t in go.tensors] == [feat_shape]
    assert bool(torch.isfinite(got).all()), "the fresh map is written in full, no memset"
    if algo == 1:
        _same(ref, got, "roi_crop_pool_bwd, LDS route")
    else:
        assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5
    _note("roi_crop_pool_bwd algo %d" % algo, gw)


@pytest.mark.parametrize("fused", [False, True], ids=["sgd_momentum_clip", "fused-fold-form"])
def test_sgd_momentum_clip(ops, fused):
    g = torch.Generator().manual_seed(4)
    sizes = [64, 4096, 70000, 12, 30000]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    total = int(offs[-1])
    w, gr, acc = torch.randn(total, generator=g), torch.randn(total, generator=g) * 0.05, torch.randn(total, generator=g) * 0.01
    gr[offs[2]:offs[3]] *= 30                                  # this variable gets clipped
    offs_t = torch.from_numpy(offs).cuda()

    def run(wd, gd, ad, offs_t):
        ops.sgd_momentum_clip(wd, gd, ad, offs_t, max(sizes), 0.01, 0.9, 10.0, zero_grads=fused)
        return wd, gd, ad
    ref = run(w.cuda(), gr.cuda(), acc.cuda(), offs_t)
    gs = GuardSet()
    upd = [gs.output(None, k, fill=v.cuda()) for k, v in (("weights", w), ("grads", gr), ("accum", acc))]   # updated in place
    with GuardedWorkspaces() as gw:
        got = run(*upd, gs.input(offs_t, "var_offsets"))
    gw.check()
    gs.check()
    assert gw.bytes_of("norms") == [ops.lib().sgd_workspace_bytes(len(sizes), max(sizes))]
    for a, b, what in zip(ref, got, ("weights", "grads", "accum")):
        _same(a, b, what)
    assert not torch.equal(got[0], w.cuda()) and (not fused or not bool(got[1].any()))
    _note("sgd_momentum_clip fused=%s" % fused, gw)


def test_prepare_images_aug_with_a_contrast_and_a_pad_slot(ops):
    """B = 3 sources, a program with one contrast slot and one mean-colour pad slot: the workspace of the mean slots is
    sized by mtlssl_prepare_images_aug_workspace and allocated by the wrapper itself (GuardedOutputs guards it)."""
    from mtl_ssl_amd import preprocessor as P
    from tests.geometric.test_gpu_detection import PROGRAMS, _planned
    codes, imgs, params, frames, tallest = _planned("crop_meanpad_contrast")
    kinds = np.asarray(codes).reshape(-1)
    slots = int((kinds == P.OP_CONTRAST).sum()) + int((kinds == P.OP_PAD).sum())
    assert (kinds == P.OP_CONTRAST).any() and (kinds == P.OP_PAD).any(), PROGRAMS["crop_meanpad_contrast"]
    OH, OW, B = 24, 40, len(imgs)
    desc, _ = ops.image_descs([a.shape[:2] for a in imgs], [False] * B, OH, OW, frames)
    d = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    px = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).cuda()
    n = len(params[0])
    prm = torch.from_numpy(np.stack(params).astype(np.float32)).cuda()
    call = lambda px, d, prm: ops.prepare_images_aug(px, d, B, OH, OW, codes, prm, n, max(tallest))
    ref, got, gw, go = _guarded_call(call, dict(px=px, d=d, prm=prm))
    nbytes = int(ops.lib().prepare_images_aug_workspace(B, slots, max(tallest)))
    assert nbytes > 0 and sorted(t.numel() * t.element_size() for t in go.tensors) == sorted([nbytes, B * OH * OW * 3 * 4])
    assert bool(torch.isfinite(got).all())
    _same(ref, got, "prepare_images_aug")
    host = [P.resize_bilinear_legacy(P.apply_program(np.float32(a), codes, p), OH, OW) for a, p in zip(imgs, params)]
    np.testing.assert_array_equal(got.cpu().numpy(), np.stack(host))
    parity_report.add("footprint prepare_images_aug B=%d, %d slots, max_H %d: workspace %d B" % (B, slots, max(tallest), nbytes))


def test_variable_histograms(ops):
    from tests.summaries.test_gpu_detection import PAD, _layout
    C = ops.HISTOGRAM_CHUNK
    sizes = [0, 1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 7]
    offsets, total = _layout(sizes)
    rng = np.random.RandomState(11)
    host = np.full(total, PAD, np.float32)
    for o, s in zip(offsets, sizes):
        host[o:o + s] = (rng.standard_normal(s) * 0.09).astype(np.float32)
    call = lambda buf: ops.variable_histograms(buf, offsets, sizes)
    (m0, c0), (m1, c1), gw, go = _guarded_call(call, dict(buf=torch.from_numpy(host).cuda()))
    tables = ops.HistogramTables(offsets, sizes, torch.device("cuda", torch.cuda.current_device()))
    assert gw.bytes_of("histograms") == [int(ops.lib().variable_histograms_workspace_bytes(tables.num_chunks))]
    assert m0.tobytes() == m1.tobytes() and c0.tobytes() == c1.tobytes()
    assert np.isfinite(m1).all() and int(c1.sum()) == sum(sizes)
    _note("variable_histograms %d chunks" % tables.num_chunks, gw)
