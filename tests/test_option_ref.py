"""CPU checks of tests/option_ref.py: the float64 adaptive-update reference against the oracle's fp32 optimizers, the
clip-boundary gradients, and the preconditions of the miner / sampler input generators that
test_gpu_option_kernels.py relies on."""
import numpy as np
import pytest

from tests import option_ref as R
from tests.f64_check import bits, within

f32 = np.float32


def _small_spec():
    return {k: R.ADAPTIVE_SPEC[k] for k in ("one", "frozen", "at_clip", "above_clip", "ragged", "zero_grad",
                                            "no_decay_big_clip")} | {"mid": ((70, 9), 1e-3, 2.0, 0.3)}


@pytest.mark.parametrize("kind,eps", [("rms_prop", 1.0), ("rms_prop", 1e-10), ("adam", 1e-8)])
def test_float64_reference_agrees_with_the_fp32_oracle(kind, eps):
    """oracle/optimizer.py runs the same update in numpy float32 with the same operation order: the gradient pipeline
    (its norm in float64 and its clip factor rounded once — inside rel_f), then the slot and weight updates, one
    rounding per operation. Its rounding count is therefore the kernel's, and adaptive_step64's own bound is the
    margin, with one difference taken out: the oracle rounds the DOUBLE difference 1 - decay to fp32 where the kernel
    subtracts in fp32, so the reference is evaluated with the oracle's constants here. The unclipped variables must
    besides equal adaptive_step32 bit for bit when that sequence is given the same constants (0.5 and 1 - 0.5)."""
    from oracle import optimizer as O
    spec = _small_spec()
    names, offs = R.layout(spec)
    rs = np.random.RandomState(7)
    h = dict(R.HYPER[kind])
    h.setdefault("p2", eps)
    wd_v = np.array([spec[n][1] for n in names], f32)
    mult_v = np.array([spec[n][2] for n in names], f32)
    sizes = {n: int(np.prod(spec[n][0])) for n in names}
    view = lambda flat: {n: flat[offs[i]:offs[i] + sizes[n]] for i, n in enumerate(names)}     # views: updated in place
    w = np.zeros(offs[-1], f32)
    for i, n in enumerate(names):
        w[offs[i]:offs[i] + sizes[n]] = rs.randn(sizes[n]) * 0.1
    s0 = np.ones_like(w) if kind == "rms_prop" else np.zeros_like(w)
    s1 = np.zeros_like(w)
    body = np.zeros(len(w), bool)                                      # the oracle knows no padding lanes
    for i, n in enumerate(names):
        body[offs[i]:offs[i] + sizes[n]] = True
    kw = dict(clip_norm=R.CLIP, weight_decay={n: float(spec[n][1]) for n in names},
              multipliers={n: float(spec[n][2]) for n in names})
    for step in range(1, 4):
        g = R.adaptive_grads(rs, spec, names, offs)
        w0, a0, b0 = w.copy(), s0.copy(), s1.copy()
        grads = view(g * f32(R.GSCALE))                                # the oracle has no loss scale: 0.5 * g is exact
        if kind == "rms_prop":
            lr = h["lr"]
            O.rmsprop_update(view(w), grads, view(s0), view(s1), lr=lr, decay=h["p0"], momentum=h["p1"], epsilon=eps, **kw)
            om = (f32(1.0 - h["p0"]), 0.0)
        else:
            lr = R.adam_lr_t(h["lr"], h["p0"], h["p1"], step)
            O.adam_update(view(w), grads, view(s0), view(s1), step=step, lr=h["lr"], beta1=h["p0"], beta2=h["p1"],
                          epsilon=eps, **kw)
            om = (f32(1.0 - h["p0"]), f32(1.0 - h["p1"]))
        ref = R.adaptive_step64(h["kind"], w0, g, a0, b0, offs, wd_v, mult_v, R.GSCALE, R.CLIP, lr, h["p0"], h["p1"],
                                h["p2"], one_minus=om)
        what = "%s eps=%g step %d: " % (kind, eps, step)
        within(s0[body], ref["s0"][body], ref["tol_s0"][body], what + "slot 0")
        within(s1[body], ref["s1"][body], ref["tol_s1"][body], what + "slot 1")
        within(w[body], ref["w"][body], ref["tol_w"][body], what + "weights")
        assert (ref["f"][offs[names.index("ragged")]] < 0.1) and (ref["f"][offs[names.index("at_clip")]] == 1.0)
        assert ref["f"][offs[names.index("above_clip")]] < 1.0
        i = names.index("frozen")
        bits(w[offs[i]:offs[i + 1]], w0[offs[i]:offs[i + 1]], what + "frozen weights")
    # the fp32 restatement with p0 = p1 = 0.5 (1 - p exact either way) is the oracle bit for bit where nothing is clipped
    w, s0, s1 = w0.copy(), np.abs(a0) + f32(0.5), np.abs(b0)
    g = R.adaptive_grads(rs, spec, names, offs)
    # adam_update forms lr_t itself: step 1 with both betas 0.5 gives lr * sqrt(0.5) / 0.5
    lr = 0.01 if kind == "rms_prop" else 0.01 * np.sqrt(1.0 - 0.5) / (1.0 - 0.5)
    wa, aa, ba = R.adaptive_step32(h["kind"], w, g, s0, s1, offs, wd_v, mult_v, R.GSCALE, lr, 0.5, 0.5, eps)
    ref = R.adaptive_step64(h["kind"], w, g, s0, s1, offs, wd_v, mult_v, R.GSCALE, R.CLIP, lr, 0.5, 0.5, eps)
    if kind == "rms_prop":
        O.rmsprop_update(view(w), view(g * f32(R.GSCALE)), view(s0), view(s1), lr=0.01, decay=0.5, momentum=0.5,
                         epsilon=eps, **kw)
    else:
        O.adam_update(view(w), view(g * f32(R.GSCALE)), view(s0), view(s1), step=1, lr=0.01, beta1=0.5, beta2=0.5,
                      epsilon=eps, **kw)
    checked = 0
    for i, n in enumerate(names):
        s = slice(offs[i], offs[i] + sizes[n])
        if ref["f"][offs[i]] == 1.0:
            bits(w[s], wa[s], "fp32 restatement, weights of " + n)
            bits(s0[s], aa[s], "fp32 restatement, slot 0 of " + n)
            bits(s1[s], ba[s], "fp32 restatement, slot 1 of " + n)
            checked += 1
    assert checked >= 5


def test_clip_boundary_gradients_in_float32():
    """The single non-zero element of `at_clip` / `above_clip`, scaled by 0.5, squared and rooted in numpy float32,
    gives the clip exactly and the next float above it — whatever the order of the (otherwise zero) sum."""
    names, offs = R.layout(R.ADAPTIVE_SPEC)
    g = R.adaptive_grads(np.random.RandomState(0), R.ADAPTIVE_SPEC, names, offs)
    clip = f32(R.CLIP)
    for name, want in (("at_clip", clip), ("above_clip", np.nextafter(clip, f32(10)))):
        i = names.index(name)
        x = g[offs[i]:offs[i + 1]] * f32(R.GSCALE)
        assert x.dtype == f32 and np.count_nonzero(x) == 1
        nrm = np.sqrt((x * x).sum(dtype=f32))
        assert nrm.dtype == f32 and nrm == want, (name, nrm, want)
    assert not (clip > clip) and np.nextafter(clip, f32(10)) > clip
    # the padding of the layout is there and belongs to the preceding variable
    assert all(o % R.ALIGN == 0 for o in offs) and offs[names.index("one") + 1] - offs[names.index("one")] == R.ALIGN
    i = names.index("zero_grad")
    assert not g[offs[i]:offs[i + 1]].any()


@pytest.mark.parametrize("with_empty", [False, True])
@pytest.mark.parametrize("n2", R.MINER_N2)
def test_miner_inputs_are_suppressed_and_tied(n2, with_empty):
    num = R.miner_num_proposals(n2, with_empty)
    loc, cls, boxes = R.miner_inputs(n2, num, seed=n2, nan_pad=False)
    assert boxes.dtype == loc.dtype == f32
    for b, n in enumerate(num):
        valid = loc[b, :n]
        assert (valid > 0).all() and (valid * 8 == np.round(valid * 8)).all()
        assert (loc[b, n:] == R.PAD_LOSS).all() and (cls[b, n:] == R.PAD_LOSS).all()
        if n >= 64:
            assert len(np.unique(valid + cls[b, :n])) < n // 2            # ties
    settings = [(0, 0.3), (64, 0.7)] if n2 > 64 else R.MINER_SETTINGS
    for nhe, iou in settings:
        if iou >= 1:
            continue
        mined = R.miner_oracle(loc, cls, boxes, num, nhe, iou, "both")
        for b, n in enumerate(num):
            assert len(mined[b]) <= n and (mined[b] < max(n, 1)).all()
            if n >= 7:                                                      # two rows of one pile among the valid ones
                assert len(mined[b]) < n, (n2, b, nhe, iou)
            if n >= 64 and nhe == 0:                                        # suppression, not the cap, removes rows
                assert n // 8 < len(mined[b]) <= n - n // 3, (n, len(mined[b]))
    nanl, nanc, _ = R.miner_inputs(n2, num, seed=n2, nan_pad=True)
    for b, n in enumerate(num):
        assert np.isnan(nanl[b, n:]).all() and np.isnan(nanc[b, n:]).all() and np.isfinite(nanl[b, :n]).all()
        bits(nanl[b, :n], loc[b, :n], "the valid rows do not depend on the padding's fill")


def test_sampler_inputs_reach_their_edges():
    c = R.sampler_mixed_batch()
    max_pos = int(c["fraction"] * c["n2"])
    cls = R.sampler_classes(c)
    assert c["ngt"][0] == 0 and cls[0][:2] == (0, 300)
    assert c["nump"][1] == 0 and c["ngt"][1] > 0
    assert cls[2][1] == 40 < c["n2"]
    assert cls[3][0] > max_pos and cls[3][1] - cls[3][0] > c["n2"]
    assert 0 < cls[4][0] < max_pos
    boxes, num, kept = R.sampler_oracle(c, seed=5)
    assert num.tolist()[:2] == [min(c["n2"], 300), 0] and num[2] <= 40 and num[3] == c["n2"] == num[4]
    assert not boxes[1].any()

    c = R.sampler_many_gt()
    for b, (npos, n, match) in enumerate(R.sampler_classes(c)):
        g = int(c["ngt"][b])
        assert n == 400 and match.max() == g - 1
        assert (match[:g] == np.arange(g)).mean() > 0.9                    # box g sits on proposal g
        if g > 256:
            assert (match >= 256).sum() >= g - 256 - 4                      # matches the LDS table could not hold
    assert c["ngt"].tolist() == [300, 257, 256, 200] and c["labels"].shape[-1] == 91

    c = R.sampler_full_table()
    assert c["props"].shape[1] == 1024 == c["nump"][0] and c["n2"] == 512
    cls = R.sampler_classes(c)
    assert cls[0][0] > int(c["fraction"] * c["n2"])                          # more positives than 128


@pytest.mark.parametrize("label_dim", [2, 21, 91])
def test_sampler_threshold_pair_is_exactly_half(label_dim):
    from oracle import boxes as OB
    c = R.sampler_threshold_case(label_dim)
    q = OB.iou(c["gts"][0, :2], c["props"][0])
    assert q.dtype == f32 and q[0, 0] == f32(0.5) and (q[1, 1:5] > 0.5).all() and not q[:, 5:].any()
    (npos, n, match), = R.sampler_classes(c)
    assert match[0] == 0 and (match[1:5] == 1).all() and (match[5:] == -1).all()
    assert npos == 1                                                         # proposal 0 only: box 1's label row is empty
    boxes, num, kept = R.sampler_oracle(c, seed=3)
    assert num[0] == 4 and 0 in kept[0].tolist()
