"""GPU: the kernels only non-default options reach — the RMSProp / Adam update, the hard-example miner, the
second-stage sampler's edges, the window dedup beyond one pass of its loops, and the elementwise helpers — each
against a float64 or exact restatement (tests/option_ref.py, checked on the CPU by tests/test_option_ref.py).

Tolerances follow from the arithmetic (eps = 2^-23): integer work, data movement and single fp32 expressions compiled
without contraction are bit-exact; the adaptive update's per-element bound is derived in option_ref's docstring; a sum
of n kept losses is within n * eps * sum|terms| of float64."""
import functools

import numpy as np
import pytest
import torch

from tests import option_ref as R
from tests import parity_report
from tests.f64_check import EPS, bits, dev, host, within

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


def _error_type():
    from mtl_ssl_amd.lib import MtlsslError
    return MtlsslError


# ------------------------------------------------------------------------------------ A. RMSProp / Adam vs float64
def _ratio(got, ref, tol):
    """Worst |got - ref| / bound over the elements that have a bound (the others were held to equality by `within`)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    live = tol > 0
    return float((err[live] / tol[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("kind,eps", [("rms_prop", 1.0), ("rms_prop", 1e-10), ("adam", 1e-8)])
def test_adaptive_update_against_float64(ops, kind, eps):
    """mtlssl_adaptive_update_clip on a ParamStore (ALIGN padding owned by the preceding variable) over three steps with
    fresh gradients, grad_scale 0.5, per-variable weight decay and multipliers (one negative: frozen), clip_norm 3.
    After every step the weights and both slots are held to the float64 evaluation of the kernel's expression on the
    DEVICE'S state before the step (bound: option_ref's docstring), and the variables the clip leaves alone also to the
    numpy float32 sequence bit for bit. Then the padding lanes, the frozen variable, the all-zero Adam variable and a
    launch without clipping on a NaN-poisoned workspace."""
    from mtl_ssl_amd import params
    assert ops.POISON_WS, "the suite hands out NaN-filled workspaces"
    spec = R.ADAPTIVE_SPEC
    h = dict(R.HYPER[kind])
    h.setdefault("p2", eps)
    K = h["kind"]
    rs = np.random.RandomState(21 + K)
    ps = params.ParamStore()
    for name, (shape, wd, *_r) in spec.items():
        ps.add(name, shape, "zeros", True, wd)
    values = {n: (rs.randn(*s[0]) * 0.1).astype(f32) for n, s in spec.items()}
    ps.finalize("cuda", values=values)
    names = [sp.name for sp in ps.trainable_specs]
    offs = host(ps.var_offsets).astype(np.int64)
    assert names == R.layout(spec)[0] and (offs == R.layout(spec)[1]).all()
    nv, total = len(names), int(offs[-1])
    sizes = [int(np.prod(spec[n][0])) for n in names]
    pad = np.ones(total, bool)
    for i in range(nv):
        pad[offs[i]:offs[i] + sizes[i]] = False
    assert pad.sum() >= 63 + 27 + 27 + 49                               # `one`, the two clip variables, `ragged`, ...
    wd_v = np.array([spec[n][1] for n in names], f32)
    mult_v = np.array([spec[n][2] for n in names], f32)
    wdt, mvt = dev(wd_v), dev(mult_v)
    slot0 = torch.ones_like(ps.weights) if kind == "rms_prop" else torch.zeros_like(ps.weights)   # trainer.py: ms = 1
    slot1 = torch.zeros_like(ps.weights)
    w_init = host(ps.weights)
    tag = "adaptive update %s eps=%g" % (kind, eps)

    def launch(w, g, s0, s1, lr, clip):
        ops.adaptive_update_clip(K, w, g, s0, s1, ps.var_offsets, ps.max_var_size, lr, h["p0"], h["p1"], h["p2"], clip,
                                 grad_scale=R.GSCALE, var_weight_decay=wdt, var_grad_mult=mvt)

    def check(before, after, g, lr, clip, what, worst):
        w0, a0, b0 = before
        ref = R.adaptive_step64(K, w0, g, a0, b0, offs, wd_v, mult_v, R.GSCALE, clip, lr, h["p0"], h["p1"], h["p2"])
        seq = R.adaptive_step32(K, w0, g, a0, b0, offs, wd_v, mult_v, R.GSCALE, lr, h["p0"], h["p1"], h["p2"])
        for key, got, s32 in zip(("w", "s0", "s1"), after, seq):
            assert np.isfinite(got).all(), "%s: non-finite %s" % (what, key)
            worst[key] = max(worst[key], _ratio(got, ref[key], ref["tol_" + key]))
            within(got, ref[key], ref["tol_" + key], "%s: %s" % (what, key))
            for i, n in enumerate(names):
                s = slice(offs[i], offs[i + 1])
                if mult_v[i] < 0:
                    bits(got[s], before[("w", "s0", "s1").index(key)][s], "%s: frozen %s" % (what, key))
                elif ref["f"][offs[i]] == 1.0:                          # left alone by the clip: the fp32 sequence itself
                    bits(got[s], s32[s], "%s: %s of unclipped %s vs the float32 sequence" % (what, key, n))
        return ref

    worst = dict(w=0.0, s0=0.0, s1=0.0)
    for step in range(1, 4):
        g = R.adaptive_grads(rs, spec, names, offs)
        ps.grads.copy_(dev(g))
        lr = h["lr"] if kind == "rms_prop" else R.adam_lr_t(h["lr"], h["p0"], h["p1"], step)
        before = tuple(host(t) for t in (ps.weights, slot0, slot1))
        launch(ps.weights, ps.grads, slot0, slot1, lr, R.CLIP)
        after = tuple(host(t) for t in (ps.weights, slot0, slot1))
        bits(host(ps.grads), g, "step %d: the gradient buffer is read only" % step)
        ref = check(before, after, g, lr, R.CLIP, "%s step %d" % (tag, step), worst)
        f = {n: ref["f"][offs[i]] for i, n in enumerate(names)}
        assert f["at_clip"] == 1.0 and f["no_decay_big_clip"] == 1.0 and f["zero_grad"] == 1.0 and f["chunk"] == 1.0
        assert 1 - 1e-6 < f["above_clip"] < 1.0 and f["ragged"] < 0.2 and f["wide"] < 1.0 and f["three_chunks_plus"] < 1.0
    w, a, b = (host(t) for t in (ps.weights, slot0, slot1))
    i = names.index("frozen")
    s = slice(offs[i], offs[i + 1])
    bits(w[s], w_init[s], "frozen weights after three steps")
    bits(a[s], np.full(offs[i + 1] - offs[i], 1.0 if kind == "rms_prop" else 0.0, f32), "frozen slot 0 after three steps")
    bits(b[s], np.zeros(offs[i + 1] - offs[i], f32), "frozen slot 1 after three steps")
    assert np.isfinite(w[pad]).all() and np.isfinite(a[pad]).all() and np.isfinite(b[pad]).all()
    assert not w[pad].any(), "the weights' padding lanes stay exactly zero"
    if kind == "adam":                                                    # 0 / (sqrt(0) + eps): no NaN, no movement
        i = names.index("zero_grad")
        s = slice(offs[i], offs[i + 1])
        bits(w[s], w_init[s], "Adam from the all-zero state with a zero gradient leaves the weights alone")
        assert not a[s].any() and not b[s].any()

    # clip_norm = 0: the norms are neither computed nor read — the workspace handed to the launch is NaN-filled
    g = R.adaptive_grads(rs, spec, names, offs)
    gd = dev(g)
    lr = h["lr"] if kind == "rms_prop" else R.adam_lr_t(h["lr"], h["p0"], h["p1"], 4)
    wc, ac, bc = ps.weights.clone(), slot0.clone(), slot1.clone()
    launch(wc, gd, ac, bc, lr, 0.0)
    worst0 = dict(w=0.0, s0=0.0, s1=0.0)
    ref = check((w, a, b), tuple(host(t) for t in (wc, ac, bc)), g, lr, 0.0, tag + " without clipping", worst0)
    assert (ref["f"] == 1.0).all()
    bits(host(gd), g, "without clipping: the gradient buffer is read only")
    for key, label in (("w", "weights"), ("s0", "slot 0"), ("s1", "slot 1")):
        parity_report.add("%s: %s worst error / bound %.3f over three clipped steps, %.3f without clipping; unclipped "
                          "variables equal the numpy float32 sequence bit for bit" % (tag, label, worst[key], worst0[key]))


def test_adaptive_update_refusals(ops):
    Err = _error_type()
    z = lambda n: torch.zeros(n, device="cuda")
    off = lambda n: torch.tensor([0, n], dtype=torch.int32, device="cuda")
    with pytest.raises(Err, match=r"adaptive_update: kind 3 \(1 RMSProp, 2 Adam\)"):
        ops.adaptive_update_clip(3, z(64), z(64), z(64), z(64), off(64), 64, 0.01, 0.9, 0.9, 1.0, 3.0)
    w = torch.ones(6, device="cuda")
    with pytest.raises(Err, match="adaptive_update: bad flat buffer size"):
        ops.adaptive_update_clip(1, w, torch.ones(6, device="cuda"), z(6), z(6), off(6), 6, 0.01, 0.9, 0.9, 1.0, 3.0)
    assert host(w).tolist() == [1.0] * 6                                  # refused before any launch


# --------------------------------------------------------------------------------- B. hard-example miner, real sizes
@functools.lru_cache(maxsize=None)
def _miner_case(n2, with_empty, nan_pad):
    num = R.miner_num_proposals(n2, with_empty)
    return (num,) + R.miner_inputs(n2, num, seed=n2 + 1000 * with_empty, nan_pad=nan_pad)


def _check_miner(ops, n2, with_empty, loss_type, nhe, iou, nan_pad):
    num, loc, cls, boxes = _miner_case(n2, with_empty, nan_pad)
    B = len(num)
    mined = R.miner_oracle(loc, cls, boxes, num, nhe, iou, loss_type)
    for b, n in enumerate(num):                                           # on the CPU, before the device is touched
        if iou < 1 and n >= 7:
            assert len(mined[b]) < n, "no suppression in image %d" % b
    box_ld, cls_ld = (360, 91) if n2 in (1, 255, 300) else (80, 21)
    rs = np.random.RandomState(n2 + nhe)
    gb, gc = rs.randn(B, n2, box_ld).astype(f32), rs.randn(B, n2, cls_ld).astype(f32)
    d_box, d_cls = dev(gb), dev(gc)
    ll, cl, sel, kept = ops.hard_example_mining(dev(loc), dev(cls), dev(boxes), dev(np.asarray(num, np.int32)), d_box, d_cls,
                                                nhe, iou, loss_type)
    ll, cl, sel, kept, d_box, d_cls = (host(t) for t in (ll, cl, sel, kept, d_box, d_cls))
    for b, n in enumerate(num):
        what = "n2=%d image %d (%d valid) %s %s" % (n2, b, n, loss_type, (nhe, iou))
        k = len(mined[b])
        assert int(kept[b]) == k, what
        assert sel[b, :k].tolist() == mined[b].tolist(), what
        keep = np.zeros(n2, bool)
        keep[mined[b]] = True
        assert not d_box[b, ~keep].any() and not d_cls[b, ~keep].any(), what + ": rows not mined are zero"
        bits(d_box[b, keep], gb[b, keep], what + ": mined box-gradient rows")
        bits(d_cls[b, keep], gc[b, keep], what + ": mined class-gradient rows")
        for got, rl, label in ((ll[b], loc[b], "localization"), (cl[b], cls[b], "classification")):
            terms = rl[mined[b]].astype(np.float64)
            if k == 0:
                assert got == 0 and not np.signbit(got), what
            within(got, terms.sum(), k * EPS * np.abs(terms).sum(), "%s: mined %s loss" % (what, label))
    assert np.isfinite(ll).all() and np.isfinite(cl).all() and np.isfinite(d_box).all() and np.isfinite(d_cls).all()


@pytest.mark.parametrize("nhe,iou", R.MINER_SETTINGS)
@pytest.mark.parametrize("loss_type", R.MINER_LOSS_TYPES)
@pytest.mark.parametrize("n2", R.MINER_N2)
def test_hard_example_miner_at_real_sizes(ops, n2, loss_type, nhe, iou):
    """ops.hard_example_mining (scores -> NMS -> apply) against oracle.frcnn_losses.hard_example_miner on the first
    num_proposals rows of each image, num_proposals = [n2, n2 // 2 + 1, min(1, n2)]: piles of near-duplicate boxes,
    tied scores, random gradients with the second stage's leading dimensions. The padding rows hold a loss above every
    real one — NaN in the (64, 0.7) setting — and boxes on top of valid ones: scored, they would be mined first."""
    _check_miner(ops, n2, False, loss_type, nhe, iou, nan_pad=(iou == 0.7))


@pytest.mark.parametrize("loss_type", R.MINER_LOSS_TYPES)
@pytest.mark.parametrize("n2", R.MINER_N2)
def test_hard_example_miner_image_without_proposals(ops, n2, loss_type):
    """num_proposals = [0, n2] with no cap on the mined count: every row of image 0 is padding the NMS appends and
    _apply must drop — nothing kept, both sums exactly 0, every gradient row zero."""
    _check_miner(ops, n2, True, loss_type, 0, 0.3, nan_pad=(loss_type == "cls"))


# ----------------------------------------------------------------------------------- C. second-stage sampler edges
def _check_sampler(ops, c, seed, what):
    H, W = c["img"]
    ob, on, num = ops.sample_proposals(dev(c["props"]), dev(c["nump"]), dev(c["gts"]), dev(c["ngt"]), dev(c["labels"]),
                                       c["n2"], c["fraction"], seed, 1, 2, H, W)
    rb, rn, kept = R.sampler_oracle(c, seed)
    assert host(num).tolist() == rn.tolist(), what
    np.testing.assert_array_equal(host(ob), rb, what)                      # the zero padding behind the counts included
    ih, iw = f32(1) / f32(H), f32(1) / f32(W)
    bits(host(on), rb * np.array([ih, iw, ih, iw], f32), what + ": boxes_norm")
    return rn, kept


@pytest.mark.parametrize("seed", [5, 77])
def test_sample_proposals_one_image_of_each_kind(ops, seed):
    """No groundtruth / no proposals / n = 40 < n2 = 64 / more positives than int(0.25 * 64) / fewer, in one batch of
    375 x 500 images; the rows behind num_proposals and num_gt hold boxes and labels that would change the result."""
    c = R.sampler_mixed_batch()
    rn, kept = _check_sampler(ops, c, seed, "mixed batch")
    assert rn[1] == 0 and rn[2] < c["n2"] and rn[3] == c["n2"]


def test_sample_proposals_full_table(ops):
    """max_p = n = SP_MAX = 1024 with n2 = 512 (and n = 1023 in the second image); one more proposal is refused."""
    c = R.sampler_full_table()
    rn, _ = _check_sampler(ops, c, 11, "1024 proposals")
    assert rn.tolist() == [512, 512]
    with pytest.raises(_error_type(), match="sample_proposals: at most 1024 proposals per image"):
        ops.sample_proposals(torch.zeros(1, 1025, 4, device="cuda"), dev(np.array([1025], np.int32)), dev(c["gts"][:1]),
                             dev(c["ngt"][:1]), dev(c["labels"][:1]), 512, 0.25, 11, 1, 2, 600, 1024)


def test_sample_proposals_groundtruth_beyond_the_lds_table(ops):
    """max_gt = 300 boxes with 91-wide label rows: the images with 300 and 257 valid boxes read groundtruth from global
    memory, the same proposals against the first 256 and 200 boxes from the LDS table; all four match the oracle."""
    c = R.sampler_many_gt()
    rn, kept = _check_sampler(ops, c, 13, "300 groundtruth boxes")
    assert rn.tolist() == [c["n2"]] * 4
    assert max(int(k.max()) for k in kept[:2]) >= 256                      # proposals matched beyond the table are sampled


@pytest.mark.parametrize("label_dim", [2, 21, 91])
def test_sample_proposals_threshold_and_background_argmax(ops, label_dim):
    """An IoU of exactly 0.5 is matched and positive; a matched box whose label row is all zeros (arg-max 0) is not."""
    c = R.sampler_threshold_case(label_dim)
    for seed in (3, 4, 9):
        rn, kept = _check_sampler(ops, c, seed, "label_dim %d seed %d" % (label_dim, seed))
        assert rn[0] == 4 and 0 in kept[0].tolist()


# --------------------------------------------------------------------------------- D. window dedup beyond one pass
def _distinct(rows):
    seen = []
    for bx in rows:
        if not any(np.array_equal(bx.view(np.uint32), s.view(np.uint32)) for s in seen):
            seen.append(bx)
    return seen


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", [2, 5])
@pytest.mark.parametrize("n2", [1, 64, 256, 300, 512])
def test_dedup_windows_is_an_exact_regrouping_at_every_size(ops, n2, E, B):
    """test_dedup_windows_is_an_exact_regrouping (tests/test_gpu_detection.py) at proposal counts below, at and beyond one
    pass of the kernel's 256-thread loops, with 2 and 5 windows and 1 and 3 images — every assertion of that test —
    and then the capacity edge on an image with five distinct last-group boxes: five slots hold them all, four flag
    the overflow and keep every row index inside its image."""
    rng = np.random.RandomState(3 + n2 + E + B)
    U = 8
    props = rng.uniform(0, 1, (B, n2, 4)).astype(f32)
    props = np.stack([np.minimum(props[..., 0], props[..., 2]), np.minimum(props[..., 1], props[..., 3]),
                      np.maximum(props[..., 0], props[..., 2]), np.maximum(props[..., 1], props[..., 3])], -1)
    if B > 1 and n2 > 200:
        props[1, 200:] = 0.0                                               # padded proposals
    ew = ops.expand_windows(dev(props), E)
    last = host(ew[:, E - 1])
    assert np.all(last[..., :2] == 0) and np.all((last[..., 2:] == 1) | (last[..., 2:] == np.nextafter(f32(1), f32(0))))
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    rois, src = ops.dedup_windows(ew, U, ovf)
    keep = (E - 1) * n2
    assert rois.shape == (B, keep + U, 4) and int(ovf.item()) == 0
    back = rois.view(-1, 4)[src.long()].view(B, E, n2, 4)
    assert torch.equal(back, ew)                                           # every window maps to an identical box
    np.testing.assert_array_equal(host(rois[:, :keep]), host(ew[:, :E - 1].reshape(B, -1, 4)))
    for b in range(B):                                                     # distinct boxes in first-occurrence order
        seen = _distinct(last[b])
        assert 1 <= len(seen) <= 4
        np.testing.assert_array_equal(host(rois[b, keep:keep + len(seen)]), np.stack(seen))
        np.testing.assert_array_equal(host(rois[b, keep + len(seen):]), np.tile(seen[0], (U - len(seen), 1)))
    # more distinct boxes than slots -> flagged
    junk = ew.clone()
    junk[0, E - 1] = torch.rand(n2, 4, device="cuda")
    ops.dedup_windows(junk, U, ovf)
    assert int(ovf.item()) == (1 if n2 > U else 0)
    if n2 < 64:
        return
    # the capacity edge: image 0's last group holds k = 5 distinct boxes spread over its n2 slots
    k = 5
    five = rng.uniform(0, 1, (k, 4)).astype(f32)
    pick = np.concatenate([rng.permutation(k), rng.randint(0, k, n2 - k)])
    w5 = ew.clone()
    w5[0, E - 1] = dev(five[pick])
    last = host(w5[:, E - 1])
    seen = [_distinct(last[b]) for b in range(B)]
    assert len(seen[0]) == k == max(len(s) for s in seen)                  # on the CPU, before the device call
    for cap in (k, k - 1):
        ovf.zero_()
        rois, src = ops.dedup_windows(w5, cap, ovf)
        R_ = keep + cap
        assert rois.shape == (B, R_, 4) and int(ovf.item()) == (0 if cap == k else 1)
        np.testing.assert_array_equal(host(rois[:, :keep]), host(w5[:, :E - 1].reshape(B, -1, 4)))
        sr = host(src).reshape(B, E * n2)
        for b in range(B):
            assert (sr[b] >= b * R_).all() and (sr[b] < (b + 1) * R_).all(), "src_row leaves image %d" % b
            n_b = min(len(seen[b]), cap)
            slots = host(rois[b, keep:])
            np.testing.assert_array_equal(slots[:n_b], np.stack(seen[b][:n_b]))
            np.testing.assert_array_equal(slots[n_b:], np.tile(seen[b][0], (cap - n_b, 1)))
        slots0 = host(rois[0, keep:]).view(np.uint32)
        assert all((slots0[s] != slots0[0]).any() for s in range(1, cap)), "a slot of image 0 repeats slot 0"
        back = host(rois.view(-1, 4)[src.long()].view(B, E, n2, 4))
        want = host(w5)
        if cap < k:                                                        # the fifth box's windows fall back to slot 0
            lost = np.array([np.array_equal(bx.view(np.uint32), seen[0][k - 1].view(np.uint32)) for bx in last[0]])
            assert lost.any()
            want[0, E - 1, lost] = seen[0][0]
        np.testing.assert_array_equal(back.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------ E. elementwise helpers, exactly
GUARD, SENTINEL = 67, f32(-12345.678)
SIZES = [1, 255, 256, 257, 65537, 2 ** 20 + 3]


def _guarded(n):
    """(buffer of n + GUARD sentinels, its first n floats as a contiguous view)."""
    buf = torch.full((n + GUARD,), float(SENTINEL), device="cuda")
    return buf, buf[:n]


def _guard_intact(buf, n, what):
    bits(host(buf[n:]), np.full(GUARD, SENTINEL, f32), what + ": guard floats behind the output")


def _values(rs, n):
    x = rs.randn(n).astype(f32)
    x[::7] *= f32(1e4)
    x[rs.randint(0, n, 3)] = (0.0, -0.0, 1e-40)[:3]
    return x


@pytest.mark.parametrize("n", SIZES)
def test_axpby_is_the_float32_expression(ops, n):
    """y = a * x + b * y as two fp32 products and one sum; b == 0 never reads y (callers pass uninitialised memory),
    also in place."""
    rs = np.random.RandomState(n % 1000)
    x, y = _values(rs, n), _values(rs, n)
    xd = dev(x)
    d = 0.9999                                                              # the EMA form axpby(w, ema, 1 - d, d)
    for a, b in ((2, -0.5), (1, 1), (0.0001, 0.9999), (1.0 - d, d)):
        buf, yv = _guarded(n)
        yv.copy_(dev(y))
        out = ops.axpby(xd, yv, a, b)
        assert out.data_ptr() == yv.data_ptr()
        bits(host(yv), f32(a) * x + f32(b) * y, "axpby n=%d a=%r b=%r" % (n, a, b))
        _guard_intact(buf, n, "axpby n=%d" % n)
    poison = np.where(np.arange(n) % 3 == 0, np.nan, np.where(np.arange(n) % 3 == 1, np.inf, -np.inf)).astype(f32)
    buf, yv = _guarded(n)
    yv.copy_(dev(poison))
    ops.axpby(xd, yv, 0.75, 0.0)
    bits(host(yv), f32(0.75) * x, "axpby n=%d with b = 0 over NaN / Inf" % n)
    _guard_intact(buf, n, "axpby b=0 n=%d" % n)
    buf, yv = _guarded(n)
    yv.copy_(xd)
    ops.axpby(yv, yv, -3.0, 0.0)                                            # in place: x is y
    bits(host(yv), f32(-3.0) * x, "axpby n=%d in place" % n)
    _guard_intact(buf, n, "axpby in place n=%d" % n)


def test_axpby_of_nothing_is_a_no_op(ops):
    buf, yv = _guarded(0)
    ops.axpby(torch.empty(0, device="cuda"), yv, 2.0, 3.0)
    ops.axpby(yv, yv, 2.0, 0.0)
    _guard_intact(buf, 0, "axpby n=0")


@pytest.mark.parametrize("shape", [(3, 3, 8, 16), (1, 1, 1088, 20), (2, 300, 4), (7,), (5, 1)])
def test_scale_channels_is_one_product_per_element(ops, shape):
    rs = np.random.RandomState(len(shape) + shape[-1])
    n = int(np.prod(shape))
    w, sc = _values(rs, n).reshape(shape), (rs.rand(shape[-1]) + 0.5).astype(f32)
    want = w * sc                                                           # the last axis is the channel
    assert want.dtype == f32
    bits(host(ops.scale_channels(dev(w), dev(sc))), want, "scale_channels %r" % (shape,))
    buf, ov = _guarded(n)
    out = ops.scale_channels(dev(w), dev(sc), out=ov.view(shape))
    assert out.data_ptr() == buf.data_ptr()
    bits(host(ov).reshape(shape), want, "scale_channels %r into out=" % (shape,))
    _guard_intact(buf, n, "scale_channels %r" % (shape,))


@pytest.mark.parametrize("n", SIZES)
def test_tanh_bwd_is_the_float32_expression(ops, n):
    rs = np.random.RandomState(n % 999)
    y = np.tanh(rs.randn(n) * 2).astype(f32)
    edge = np.array([1.0, -1.0, 0.0, 1e-40], f32)
    assert edge[3] != 0 and edge[3] < np.finfo(f32).tiny                    # a subnormal
    y[:min(n, 4)] = edge[:min(n, 4)]
    if n >= 8:
        y[-4:] = edge[::-1]
    dy = _values(rs, n)
    want = dy * (f32(1) - y * y)
    assert want.dtype == f32
    bits(host(ops.tanh_bwd(dev(y), dev(dy))), want, "tanh_bwd n=%d" % n)
    buf, dx = _guarded(n)                                                   # the C entry point on a guarded output
    yd, dyd = dev(y), dev(dy)
    ops.lib().tanh_bwd(ops.ptr(yd), ops.ptr(dyd), ops.ptr(dx), n, ops._stream())
    torch.cuda.synchronize()
    bits(host(dx), want, "tanh_bwd n=%d into a guarded buffer" % n)
    _guard_intact(buf, n, "tanh_bwd n=%d" % n)
