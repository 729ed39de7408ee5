"""References and input generators of the option-kernel tests (test_gpu_option_kernels.py, checked on the CPU by
test_option_ref.py): the float64 restatement of mtlssl_adaptive_update_clip (RMSProp / Adam) with its per-element
error bound, the same sequence in numpy float32 for the bit comparison, and the inputs of the hard-example-miner and
second-stage-sampler cases. A plain module: no fixtures, not a conftest.

The error bound of the adaptive update (u = EPS / 2 is the fp32 unit roundoff; every count is first order in u, and
the bounds are multiplied by 1 + 1e-6 for the terms in u^2):

  gradient pipeline  gg = ((g * gscale + wd * w) * mult) * f
      two products (u of each), their sum (u * |sum| <= u * (|g gscale| + |wd w|)), two more products (2u):
          d_g = 4u * G + |gg| * rel_f = 2 EPS * G + |gg| * rel_f,    G = (|g gscale| + |wd w|) * |mult| * f
      f = clip / max(norm, clip). When the variable is clipped, the norm is a sum of non-negative squares reduced over
      `depth` additions (4 squares per float4, min(n, 64k) / 1024 float4 per lane, 6 wave levels, 2 across the waves,
      the chunks in order), so it is within depth * u relative; the other depth * u of rel_f = depth * EPS cover the
      roundings of the squared elements (4u each, halved by the root), the root and the quotient (depth >= 13 > 6).

  a sum of two products t1 + t2, each product rounded once: u |t1| + u |t2| + u |t1 + t2| <= EPS * (|t1| + |t2|).

  RMSProp   ms'  = p0 * ms + ((1 - p0) * gg) * gg      t2 carries two more roundings (1 - p0, the second product)
                   tol_ms  = EPS * (|t1| + 2 |t2|) + 2 (1 - p0) |gg| d_g
            q    = (lr * gg) / sqrt(ms' + eps)         s = ms' + eps is off by tol_ms + u s, the root halves the relative
                                                       error and adds u, the product and the quotient add u each
                   tol_q   = |q| * (3u + rho_s / 2) + lr d_g / sqrt(s),     rho_s = (tol_ms + u s) / s
            mom' = p1 * mom + q                        tol_mom = EPS * (|p1 mom| + |q|) + tol_q
            w'   = w - mom'                            tol_w   = EPS * (|w| + |mom'|) + tol_mom
  Adam      m'   = p0 * m + (1 - p0) * gg              t2 carries one more rounding (1 - p0)
                   tol_m   = EPS * (|t1| + 1.5 |t2|) + (1 - p0) d_g
            v'   = p1 * v + ((1 - p1) * gg) * gg       tol_v   = EPS * (|t1| + 2 |t2|) + 2 (1 - p1) |gg| d_g
            den  = sqrt(v') + eps                      |sqrt(x) - sqrt(y)| <= |x - y| / sqrt(y); the root and the sum add
                                                       u each:  e_den = tol_v / sqrt(v') + u sqrt(v') + u den
            q    = (lr * m') / den                     tol_q   = (lr tol_m + u |lr m'|) / (den - e_den)
                                                                 + |q| e_den / (den - e_den) + u |q|
            w'   = w - q                               tol_w   = EPS * (|w| + |q|) + tol_q
"""
import numpy as np

from tests.f64_check import EPS

f32 = np.float32
ALIGN = 64                      # mtl_ssl_amd/params.py: every variable starts on a multiple of 64 floats
CH = 1 << 16                    # NORM_CHUNK of csrc/ops.hip
CLIP, GSCALE = 3.0, 0.5

# name: (shape, weight decay, multiplier, gradient std) — the variables of the momentum test
# (test_sgd_momentum_clip_fold_and_bn_refresh_against_float64) and two more
ADAPTIVE_SPEC = {
    "one": ((1,), 0.0, 1.0, 1.0),
    "below_chunk": ((CH - 64,), 4e-5, 1.0, 0.02),
    "chunk": ((1024, 64), 0.0, 2.0, 0.01),
    "three_chunks_plus": ((3073, 64), 1e-3, 0.5, 0.03),      # 3 x 65 536 + 64
    "frozen": ((10, 100), 1e-3, -1.0, 1.0),
    "wide": ((97, 2048), 0.0, 1.0, 0.05),
    "at_clip": ((37,), 0.0, 1.0, 0.0),                       # norm == clip to the last bit
    "above_clip": ((37,), 0.0, 1.0, 0.0),                    # norm one ulp above clip
    "ragged": ((5, 3), 2e-4, 1.5, 0.4),                      # clipped hard
    "zero_grad": ((130,), 0.0, 1.0, 0.0),                    # gradient identically zero, no decay
    "no_decay_big_clip": ((300,), 0.0, 1.0, 0.05),           # norm ~ 0.4: far below the clip, f = 1
}
# the scalars of the three optimizers under test (p0, p1, p2 as mtlssl_adaptive_update_clip names them)
HYPER = {
    "rms_prop": dict(kind=1, lr=0.01, p0=0.9, p1=0.9),       # decay, momentum; epsilon per case
    "adam": dict(kind=2, lr=0.01, p0=0.9, p1=0.999, p2=1e-8),
}


def adam_lr_t(lr, beta1, beta2, t):
    """The step size the caller forms (mtl_ssl_amd/trainer.py, apply_gradients), t counting from 1."""
    return lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)


def layout(spec):
    """(names, offsets int64 [nv + 1]) of a ParamStore holding `spec` in order: ALIGN padding belongs to the
    preceding variable."""
    names, offs = list(spec), [0]
    for n in names:
        offs.append(offs[-1] + -(-int(np.prod(spec[n][0])) // ALIGN) * ALIGN)
    return names, np.asarray(offs, np.int64)


def adaptive_grads(rs, spec, names, offs):
    """One step's gradient buffer (padding lanes zero). `at_clip` / `above_clip` hold one non-zero element each:
    (g * 0.5) ** 2 = 9 and (next float above 3) ** 2, so sqrtf of the fp32 sum of squares is 3 exactly / one ulp more."""
    g = np.zeros(int(offs[-1]), f32)
    for i, n in enumerate(names):
        sz = int(np.prod(spec[n][0]))
        g[offs[i]:offs[i] + sz] = rs.randn(sz) * spec[n][3]
    if "at_clip" in spec:
        g[offs[names.index("at_clip")] + 5] = 6.0
    if "above_clip" in spec:
        g[offs[names.index("above_clip")] + 11] = 2 * np.nextafter(f32(CLIP), f32(10))
    if "ragged" in spec:
        i = names.index("ragged")
        g[offs[i]:offs[i] + 15] *= 40
    return g


def norm_depth(n):
    """Longest chain of additions a square passes through in k_var_sumsq / k_var_norm_fold for a variable of n floats."""
    return 4 * -(-min(n, CH) // 1024) + 6 + 2 + -(-n // CH)


def adaptive_step64(kind, w, g, s0, s1, offs, wd_v, mult_v, gscale, clip, lr, p0, p1, p2, one_minus=None):
    """The kernel's expression in float64 from the fp32 state before the step and the fp32 scalars the C ABI receives.
    -> dict(w, s0, s1: float64 results; tol_w, tol_s0, tol_s1: per-element bounds (module docstring); f: the clip
    factor per element). `one_minus`: (1 - p0, 1 - p1) as another fp32 implementation forms them (oracle/optimizer.py
    rounds the double difference), instead of the kernel's 1.f - p0."""
    w, g, a, b = (np.asarray(x, f32).astype(np.float64) for x in (w, g, s0, s1))
    gscale, clip, lr, p0, p1, p2 = (float(f32(x)) for x in (gscale, clip, lr, p0, p1, p2))
    q0, q1 = (1.0 - p0, 1.0 - p1) if one_minus is None else (float(one_minus[0]), float(one_minus[1]))
    total, u = len(w), EPS / 2
    gg, G, f_all, rel_f, live = np.zeros(total), np.zeros(total), np.ones(total), np.zeros(total), np.zeros(total, bool)
    for i in range(len(offs) - 1):
        s = slice(int(offs[i]), int(offs[i + 1]))                     # the padding belongs to variable i
        m = float(f32(mult_v[i]))
        if m < 0:
            continue                                                    # frozen: not in apply_gradients
        live[s] = True
        gs, t = g[s] * gscale, float(f32(wd_v[i])) * w[s]
        x = (gs + t) * m
        f = 1.0
        if clip > 0:
            f = clip / max(float(np.sqrt((x * x).sum())), clip)        # tf.clip_by_norm
        gg[s], G[s], f_all[s] = x * f, (np.abs(gs) + np.abs(t)) * abs(m) * f, f
        if f < 1:
            rel_f[s] = norm_depth(int(offs[i + 1] - offs[i])) * EPS
    d_g = 2 * EPS * G + np.abs(gg) * rel_f
    ag = np.abs(gg)
    if kind == 1:
        t1, t2 = p0 * a, q0 * gg * gg
        a2 = t1 + t2
        tol_a = EPS * (np.abs(t1) + 2 * np.abs(t2)) + 2 * q0 * ag * d_g
        sm = np.where(live, a2 + p2, 1.0)
        assert (sm > 0).all(), "the mean-square slot must stay positive"
        den = np.sqrt(sm)
        rho = (tol_a + u * sm) / sm
        q = lr * gg / den
        tol_q = np.abs(q) * (3 * u + rho / 2) + lr * d_g / den
        t1b = p1 * b
        b2 = t1b + q
        tol_b = EPS * (np.abs(t1b) + np.abs(q)) + tol_q
        w2 = w - b2
        tol_w = EPS * (np.abs(w) + np.abs(b2)) + tol_b
    else:
        t1, t2 = p0 * a, q0 * gg
        a2 = t1 + t2
        tol_a = EPS * (np.abs(t1) + 1.5 * np.abs(t2)) + q0 * d_g
        u1, u2 = p1 * b, q1 * gg * gg
        b2 = u1 + u2
        assert (b2[live] >= 0).all(), "Adam's second moment must stay non-negative"
        tol_b = EPS * (np.abs(u1) + 2 * np.abs(u2)) + 2 * q1 * ag * d_g
        r = np.sqrt(np.where(live, b2, 0.0))
        den = r + p2
        e_den = np.where(r > 0, tol_b / np.where(r > 0, r, 1.0), 0.0) + u * r + u * den
        lo = den - e_den
        assert (lo[live] > 0).all(), "Adam's denominator is not resolved by fp32 at these inputs"
        lo = np.where(live, lo, 1.0)
        num = lr * a2
        q = num / np.where(live, den, 1.0)
        tol_q = (lr * tol_a + u * np.abs(num)) / lo + np.abs(q) * e_den / lo + u * np.abs(q)
        w2 = w - q
        tol_w = EPS * (np.abs(w) + np.abs(q)) + tol_q
    keep = lambda new, old: np.where(live, new, old)
    zero = lambda t: np.where(live, t * (1 + 1e-6), 0.0)          # the counts above are first order in u = 6e-8
    return dict(w=keep(w2, w), s0=keep(a2, a), s1=keep(b2, b), tol_w=zero(tol_w), tol_s0=zero(tol_a), tol_s1=zero(tol_b),
                f=f_all)


def adaptive_step32(kind, w, g, s0, s1, offs, wd_v, mult_v, gscale, lr, p0, p1, p2):
    """The kernel's sequence in numpy float32 for an unclipped variable (f = 1, a multiplication that changes nothing):
    one IEEE operation per kernel operation, no contraction, 1 - p0 formed in float32. -> (w, s0, s1)."""
    w, g, a, b = (np.array(x, f32) for x in (w, g, s0, s1))
    gscale, lr, p0, p1, p2, one = (f32(x) for x in (gscale, lr, p0, p1, p2, 1.0))
    for i in range(len(offs) - 1):
        s = slice(int(offs[i]), int(offs[i + 1]))
        m = f32(mult_v[i])
        if m < 0:
            continue
        gg = (g[s] * gscale + f32(wd_v[i]) * w[s]) * m
        if kind == 1:
            a[s] = p0 * a[s] + (one - p0) * gg * gg
            b[s] = p1 * b[s] + lr * gg / np.sqrt(a[s] + p2)
            w[s] = w[s] - b[s]
        else:
            a[s] = p0 * a[s] + (one - p0) * gg
            b[s] = p1 * b[s] + (one - p1) * gg * gg
            w[s] = w[s] - lr * a[s] / (np.sqrt(b[s]) + p2)
    assert w.dtype == a.dtype == b.dtype == f32
    return w, a, b


# ------------------------------------------------------------------------------------------- hard-example miner
IMG_H, IMG_W = 600.0, 1024.0
MINER_N2 = (1, 64, 255, 256, 257, 300, 512)
MINER_LOSS_TYPES = ("both", "cls", "loc")
MINER_SETTINGS = ((0, 0.3), (1, 0.5), (64, 0.7), (64, 1.0))      # (num_hard_examples, iou_threshold)
PAD_LOSS = 100.0                                                  # above every real loss: a padding row that is scored wins


def miner_num_proposals(n2, with_empty):
    return [0, n2] if with_empty else [n2, n2 // 2 + 1, min(1, n2)]


def miner_inputs(n2, num_proposals, seed, nan_pad):
    """-> (loc [B,n2], cls [B,n2], boxes [B,n2,4]). Every second row sits on one of three piles of near-duplicates
    (jitter of a pixel on boxes of 100+ pixels: IoU ~ 0.97), the others are scattered over the image. The losses are
    positive multiples of 1/8 (<= 2), so many scores tie and the order among ties is part of the result. Rows at and
    behind num_proposals[b] — the padding — continue the same box pattern (so they overlap valid rows) and hold a loss
    of NaN (`nan_pad`) or PAD_LOSS."""
    rs = np.random.RandomState(seed)
    B = len(num_proposals)
    piles = np.array([[100, 100, 300, 400], [250, 500, 420, 760], [50, 600, 500, 900]], np.float64)
    boxes = np.zeros((B, n2, 4), f32)
    for b in range(B):
        cy, cx = rs.uniform(60, IMG_H - 60, n2), rs.uniform(60, IMG_W - 60, n2)
        h, w = rs.uniform(40, 240, n2), rs.uniform(40, 240, n2)
        bx = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1)
        i = np.arange(0, n2, 2)
        bx[i] = piles[(i // 2) % 3] + rs.uniform(-1, 1, (len(i), 4))
        boxes[b] = bx
    loc = (rs.randint(1, 17, (B, n2)) / 8.0).astype(f32)
    cls = (rs.randint(1, 17, (B, n2)) / 8.0).astype(f32)
    for b in range(B):
        loc[b, num_proposals[b]:] = np.nan if nan_pad else PAD_LOSS
        cls[b, num_proposals[b]:] = np.nan if nan_pad else PAD_LOSS
    return loc, cls, boxes


def miner_oracle(loc, cls, boxes, num_proposals, num_hard_examples, iou_threshold, loss_type):
    """oracle.frcnn_losses.hard_example_miner per image on the first num_proposals[b] rows (the reference's unpad
    step). -> [kept indices per image]."""
    from oracle import frcnn_losses as L
    mined = []
    for b, n in enumerate(num_proposals):
        if n == 0:
            mined.append(np.zeros(0, np.int32))
            continue
        _, _, m = L.hard_example_miner([loc[b, :n]], [cls[b, :n]], [boxes[b, :n]], num_hard_examples, iou_threshold,
                                       loss_type)
        mined.append(np.asarray(m[0], np.int32))
    return mined


# -------------------------------------------------------------------------------------------- second-stage sampler
def random_boxes(rs, n, img_h, img_w, lo=16.0, hi=200.0):
    cy, cx = rs.uniform(0, img_h, n), rs.uniform(0, img_w, n)
    h, w = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n)
    b = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], 1)
    return np.clip(b, 0, [img_h, img_w, img_h, img_w]).astype(f32)


def one_hot_labels(rs, g, label_dim):
    lab = np.zeros((g, label_dim), f32)
    lab[np.arange(g), 1 + rs.randint(0, label_dim - 1, g)] = 1
    return lab


def sampler_mixed_batch(label_dim=21, seed=31):
    """One image of each kind, n2 = 64, balance fraction 0.25 (at most 16 positives), 375 x 500 images:
    0 no groundtruth, 1 no proposals, 2 n = 40 < n2, 3 more positives than 16, 4 fewer positives than 16. Rows behind
    num_proposals / num_gt hold live-looking boxes and foreground labels: reading them changes the result."""
    rs = np.random.RandomState(seed)
    H, W, B, max_p, G = 375.0, 500.0, 5, 300, 6
    props = np.stack([random_boxes(rs, max_p, H, W) for _ in range(B)])
    nump = np.array([300, 0, 40, 300, 290], np.int32)
    ngt = np.array([0, 3, 4, 5, 2], np.int32)
    gts = np.stack([props[b, 3:3 + G] + rs.uniform(-1, 1, (G, 4)).astype(f32) for b in range(B)]).astype(f32)
    labels = np.stack([one_hot_labels(rs, G, label_dim) for _ in range(B)])
    for b, count in ((2, 6), (3, 12), (4, 2)):                      # proposals piled onto the image's valid boxes
        for g in range(ngt[b]):
            lo = 20 + g * count if b != 2 else 8 + g * count
            props[b, lo:lo + count] = gts[b, g] + rs.uniform(-2, 2, (count, 4)).astype(f32)
    return dict(props=props, nump=nump, gts=gts, ngt=ngt, labels=labels, n2=64, fraction=0.25, img=(H, W))


def sampler_many_gt(seed=32, label_dim=91):
    """The same 400 of 512 proposals against the first 300 / 257 / 256 / 200 of 300 groundtruth boxes (one image each):
    box g sits on proposal g, so proposals 256..299 match boxes beyond the 256 that fit the kernel's LDS table."""
    rs = np.random.RandomState(seed)
    H, W, max_p, G = 600.0, 1024.0, 512, 300
    p = random_boxes(rs, max_p, H, W, 30.0, 120.0)
    gt = (p[:G] + rs.uniform(-1, 1, (G, 4))).astype(f32)
    lab = one_hot_labels(rs, G, label_dim)
    ngt = np.array([300, 257, 256, 200], np.int32)
    B = len(ngt)
    return dict(props=np.stack([p] * B), nump=np.full(B, 400, np.int32), gts=np.stack([gt] * B), ngt=ngt,
                labels=np.stack([lab] * B), n2=128, fraction=0.5, img=(H, W))


def sampler_full_table(seed=33, label_dim=21):
    """max_p = n = 1024 (the kernel's table size) with n2 = 512."""
    rs = np.random.RandomState(seed)
    H, W, B, max_p, G = 600.0, 1024.0, 2, 1024, 8
    props = np.stack([random_boxes(rs, max_p, H, W) for _ in range(B)])
    gts = np.stack([props[b, 1000:1000 + G] + rs.uniform(-1, 1, (G, 4)).astype(f32) for b in range(B)]).astype(f32)
    for b in range(B):
        for g in range(G):
            props[b, 100 + 30 * g:130 + 30 * g] = gts[b, g] + rs.uniform(-3, 3, (30, 4)).astype(f32)
    return dict(props=props, nump=np.array([1024, 1023], np.int32), gts=gts, ngt=np.array([G, G - 1], np.int32),
                labels=np.stack([one_hot_labels(rs, G, label_dim) for _ in range(B)]), n2=512, fraction=0.25, img=(H, W))


def sampler_threshold_case(label_dim, seed=34):
    """Proposal 0 = [0, 0, 10, 10] against box 0 = [0, 0, 10, 5]: intersection 50, union 100 + 50 - 50, IoU 0.5 exactly —
    matched (the matcher asks `not 0.5 > iou`) and, box 0 being a foreground box, positive. Proposals 1..4 sit on box 1,
    whose label row is all zeros: matched, arg-max 0, not positive. The rest are far away. n2 = 4 with fraction 0.5: the
    one positive is always sampled, three of the eleven others follow by priority."""
    rs = np.random.RandomState(seed)
    H, W = 375.0, 500.0
    props = np.zeros((1, 12, 4), f32)
    props[0, 0] = [0, 0, 10, 10]
    props[0, 1:5] = np.array([100, 100, 200, 220], f32) + rs.uniform(-2, 2, (4, 4)).astype(f32)
    props[0, 5:] = random_boxes(rs, 7, H, W) + f32(240)
    gts = np.array([[[0, 0, 10, 5], [100, 100, 200, 220], [0, 0, 0, 0]]], f32)
    labels = np.zeros((1, 3, label_dim), f32)
    labels[0, 0, label_dim - 1] = 1
    labels[0, 2, 1] = 1                                               # behind num_gt
    return dict(props=props, nump=np.array([12], np.int32), gts=gts, ngt=np.array([2], np.int32), labels=labels, n2=4,
                fraction=0.5, img=(H, W))


def sampler_oracle(c, seed):
    """oracle.frcnn_losses.sample_box_classifier_batch on a case of the generators above -> (boxes, num, kept)."""
    from oracle import frcnn_losses as L
    B = len(c["nump"])
    return L.sample_box_classifier_batch(c["props"], c["nump"], [c["gts"][b, :c["ngt"][b]] for b in range(B)],
                                         [c["labels"][b, :c["ngt"][b]] for b in range(B)], c["n2"], c["fraction"], seed)


def sampler_classes(c):
    """Per image (number of positives, number of valid proposals) as the oracle's assigner sees them."""
    from oracle import assign as A
    out = []
    for b in range(len(c["nump"])):
        n, g = int(c["nump"][b]), int(c["ngt"][b])
        unmatched = np.zeros(c["labels"].shape[-1], f32)
        unmatched[0] = 1
        r = A.assign_targets(c["props"][b, :n], c["gts"][b, :g], c["labels"][b, :g], unmatched, 0.5)
        out.append((int((np.argmax(r["cls_targets"], 1) > 0).sum()) if n else 0, n, r["match"]))
    return out
