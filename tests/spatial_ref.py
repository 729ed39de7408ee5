"""float64 NumPy restatements of the spatial operations between trunk and heads (test infrastructure).

Design rule: whatever DECIDES AN INDEX (a sampling coordinate, its validity, floor / ceil, the interpolation fraction)
is restated in float32, one correctly rounded operation per step and in the order TF 1.7 and the kernels use, so the
reference picks the same taps as the code under test by construction; only the VALUE arithmetic is float64, with the
float32 fractions widened. ops.hip is compiled with -ffp-contract=off (mtl_ssl_amd/build.py SOURCES), so the kernels'
coordinate arithmetic is exactly this sequence of individually rounded operations.

Every reference also returns what an error bound needs: the magnitude of the operands per output element (max |corner|
of a blend, sum |term| of a sum) and, for scatters and gathers, the number of contributions per element.

All maps are NHWC like the reference project. Nothing is read from the reference tree at run time; the citations name
the files these formulas come from (TensorFlow 1.7 is the reference's pinned third-party dependency)."""
import numpy as np

f32 = np.float32
f64 = np.float64


def same_pad(n, k, stride, dilation=1):
    """TF 'SAME': (pad_before, out); the odd pixel of padding goes at the end."""
    k_eff = (k - 1) * dilation + 1
    out = -(-n // stride)
    total = max((out - 1) * stride + k_eff - n, 0)
    return total // 2, out


def pool_geometry(H, W, k, stride, padding):
    if padding == "SAME":
        pt, OH = same_pad(H, k, stride)
        pl, OW = same_pad(W, k, stride)
        return pt, pl, OH, OW
    return 0, 0, (H - k) // stride + 1, (W - k) // stride + 1


# ------------------------------------------------------------------------------------------------ crop_and_resize
def crop_axis(lo, hi, n, crop):
    """Sampling positions of tf.image.crop_and_resize along one axis (TF 1.7 crop_and_resize_op.cc, CropAndResize
    functor; call site faster_rcnn_meta_arch.py:1340-1344) in float32, step by step:
        crop > 1:  scale = (hi - lo) * (n - 1) / (crop - 1);  pos = lo * (n - 1) + i * scale
        crop == 1: pos = 0.5 * (lo + hi) * (n - 1)
        valid = !(pos < 0 || pos > n - 1);  i0 = floor(pos), i1 = ceil(pos), frac = pos - floor(pos).
    lo, hi: float32 [R] -> pos float32 [R,crop], valid bool, i0 / i1 int64 (clamped into the map where the sample is
    invalid, so that they can index), frac float32."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    nm1 = f32(n - 1)
    if crop > 1:
        scale = ((hi - lo) * nm1) / f32(crop - 1)
        pos = (lo * nm1)[:, None] + np.arange(crop, dtype=f32)[None, :] * scale[:, None]
    else:
        pos = ((f32(0.5) * (lo + hi)) * nm1)[:, None]
    assert pos.dtype == f32
    valid = ~((pos < f32(0)) | (pos > nm1))
    fl, ce = np.floor(pos), np.ceil(pos)
    frac = pos - fl
    assert frac.dtype == f32
    i0 = np.clip(np.where(valid, fl, 0), 0, n - 1).astype(np.int64)
    i1 = np.clip(np.where(valid, ce, 0), 0, n - 1).astype(np.int64)
    return pos, valid, i0, i1, frac


def crop_and_resize(feat, boxes, box_ind, crop, chunk=64):
    """tf.image.crop_and_resize (bilinear, extrapolation_value 0). feat float32 [B,H,W,C]; boxes float32 [R,4]
    (y1,x1,y2,x2) normalised; crop int or (ch, cw). -> (val, amax, valid): val float64 [R,ch,cw,C] = top + (bot-top)*yl
    with top = tl + (tr-tl)*xl, bot = bl + (br-bl)*xl, 0 where the sample is extrapolated; amax = max |corner| per
    element (0 where extrapolated); valid bool [R,ch,cw]."""
    ch, cw = (crop, crop) if isinstance(crop, int) else crop
    B, H, W, C = feat.shape
    boxes = np.asarray(boxes, f32)
    box_ind = np.asarray(box_ind, np.int64)
    R = boxes.shape[0]
    _, vy, ty, by, yl = crop_axis(boxes[:, 0], boxes[:, 2], H, ch)
    _, vx, lx, rx, xl = crop_axis(boxes[:, 1], boxes[:, 3], W, cw)
    val = np.zeros((R, ch, cw, C), f64)
    amax = np.zeros((R, ch, cw, C), f64)
    valid = vy[:, :, None] & vx[:, None, :]
    for a in range(0, R, chunk):
        s = slice(a, min(a + chunk, R))
        bi = box_ind[s, None, None]

        def g(yy, xx):
            return feat[bi, yy[s, :, None], xx[s, None, :]].astype(f64)
        tl, tr, bl, br = g(ty, lx), g(ty, rx), g(by, lx), g(by, rx)
        xw = xl[s].astype(f64)[:, None, :, None]
        yw = yl[s].astype(f64)[:, :, None, None]
        top = tl + (tr - tl) * xw
        bot = bl + (br - bl) * xw
        ok = valid[s][..., None]
        val[s] = np.where(ok, top + (bot - top) * yw, 0.0)
        amax[s] = np.where(ok, np.maximum(np.maximum(np.abs(tl), np.abs(tr)), np.maximum(np.abs(bl), np.abs(br))), 0.0)
    return val, amax, valid


def pool_windows(v, pk, ps):
    """VALID pk x pk / ps windows of the crops (the max-pool the reference applies right after the crop,
    faster_rcnn_meta_arch.py:1345-1348): v [R,ch,cw,C] -> [R,PH,PW,pk*pk,C], window positions in (dy, dx) order."""
    R, ch, cw, C = v.shape
    PH, PW = (ch - pk) // ps + 1, (cw - pk) // ps + 1
    out = np.empty((R, PH, PW, pk * pk, C), v.dtype)
    for dy in range(pk):
        for dx in range(pk):
            out[:, :, :, dy * pk + dx] = v[:, dy:dy + (PH - 1) * ps + 1:ps, dx:dx + (PW - 1) * ps + 1:ps]
    return out


def roi_crop_pool_bwd(dout, sel, feat_shape, boxes, box_ind, crop, pk, ps):
    """Gradient of max-pool(crop_and_resize) with respect to the map, as a float64 scatter. dout float32 [R,PH,PW,C];
    sel integer [R,PH,PW,C]: the window position (dy*pk+dx) that took each maximum (None = position 0, for pk == 1).
    The sample (cy, cx) = (py*ps+dy, px*ps+dx), if valid, sends g*(1-yl)*(1-xl), g*(1-yl)*xl, g*yl*(1-xl), g*yl*xl to
    (ty,lx), (ty,rx), (by,lx), (by,rx) (crop_and_resize_op.cc CropAndResizeBackpropImage).
    -> (grad, n, sabs) float64 / int64 / float64 [B,H,W,C]: the sum, the number of non-zero contributions and the sum
    of their absolute values per map element."""
    B, H, W, C = feat_shape
    boxes = np.asarray(boxes, f32)
    box_ind = np.asarray(box_ind, np.int64)
    R, PH, PW, _ = dout.shape
    _, vy, ty, by, yl = crop_axis(boxes[:, 0], boxes[:, 2], H, crop)
    _, vx, lx, rx, xl = crop_axis(boxes[:, 1], boxes[:, 3], W, crop)
    sel = np.zeros(dout.shape, np.int64) if sel is None else np.asarray(sel, np.int64)
    r = np.arange(R)[:, None, None, None]
    cy = (np.arange(PH) * ps)[None, :, None, None] + sel // pk
    cx = (np.arange(PW) * ps)[None, None, :, None] + sel % pk
    ok = vy[r, cy] & vx[r, cx]
    g = np.where(ok, dout.astype(f64), 0.0)
    wy1, wx1 = yl.astype(f64)[r, cy], xl.astype(f64)[r, cx]
    base = box_ind[:, None, None, None] * H
    ch = np.broadcast_to(np.arange(C)[None, None, None, :], dout.shape)
    size = B * H * W * C
    grad, n, sabs = np.zeros(size), np.zeros(size, np.int64), np.zeros(size)
    for yy, wy in ((ty[r, cy], 1.0 - wy1), (by[r, cy], wy1)):
        for xx, wx in ((lx[r, cx], 1.0 - wx1), (rx[r, cx], wx1)):
            c = g * wy * wx
            idx = (((base + yy) * W + xx) * C + ch).ravel()
            cr = c.ravel()
            grad += np.bincount(idx, cr, size)
            sabs += np.bincount(idx, np.abs(cr), size)
            n += np.bincount(idx, (cr != 0).astype(f64), size).astype(np.int64)
    return grad.reshape(feat_shape), n.reshape(feat_shape), sabs.reshape(feat_shape)


# ---------------------------------------------------------------------------------------- position-sensitive RoI
def psroi_axis(lo, hi, n, bins, bs):
    """Sub-box arithmetic of ops.position_sensitive_crop_regions (object_detection/utils/ops.py:462-609) along one
    axis, in float32: step = (hi - lo) / bins; bin b spans [lo + b*step, lo + (b+1)*step] and is sampled by
    crop_and_resize at bs points. -> per bin the crop_axis tuple, stacked: valid / i0 / i1 / frac [R,bins,bs]."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    step = (hi - lo) / f32(bins)
    out = [crop_axis(lo + f32(b) * step, lo + f32(b + 1) * step, n, bs)[1:] for b in range(bins)]
    return tuple(np.stack([o[k] for o in out], 1) for k in range(4))


def psroi(fmap, boxes, box_ind, crop, bins):
    """position_sensitive_crop_regions(global_pool=True) (utils/ops.py:462-609; call sites
    core/box_predictor.py:229-256): bin (by,bx) crops ITS channel group g = by*bins_x+bx of the score map at
    bs_y x bs_x points; the result is the mean over bins and samples (extrapolated samples count as 0).
    fmap float32 [B,H,W,nb*Cc] -> (val float64 [R,Cc], sumA float64 [R,Cc]: sum over the valid samples of max |corner|)."""
    B, H, W, Ct = fmap.shape
    nb = bins[0] * bins[1]
    Cc = Ct // nb
    bs = (crop[0] // bins[0], crop[1] // bins[1])
    boxes = np.asarray(boxes, f32)
    box_ind = np.asarray(box_ind, np.int64)
    R = boxes.shape[0]
    vy, ty, by, yl = psroi_axis(boxes[:, 0], boxes[:, 2], H, bins[0], bs[0])
    vx, lx, rx, xl = psroi_axis(boxes[:, 1], boxes[:, 3], W, bins[1], bs[1])
    val, sumA = np.zeros((R, Cc)), np.zeros((R, Cc))
    bi = box_ind[:, None, None]
    for b0 in range(bins[0]):
        for b1 in range(bins[1]):
            gsl = slice((b0 * bins[1] + b1) * Cc, (b0 * bins[1] + b1 + 1) * Cc)
            fm = fmap[..., gsl]

            def g(yy, xx):
                return fm[bi, yy[:, b0, :, None], xx[:, b1, None, :]].astype(f64)
            tl, tr, bl, br = g(ty, lx), g(ty, rx), g(by, lx), g(by, rx)
            xw = xl[:, b1].astype(f64)[:, None, :, None]
            yw = yl[:, b0].astype(f64)[:, :, None, None]
            top = tl + (tr - tl) * xw
            bot = bl + (br - bl) * xw
            ok = (vy[:, b0, :, None] & vx[:, b1, None, :])[..., None]
            val += np.where(ok, top + (bot - top) * yw, 0.0).sum((1, 2))
            sumA += np.where(ok, np.maximum(np.maximum(np.abs(tl), np.abs(tr)), np.maximum(np.abs(bl), np.abs(br))),
                             0.0).sum((1, 2))
    cnt = nb * bs[0] * bs[1]
    return val / cnt, sumA / cnt


def _axis_weights(valid, i0, i1, frac, n):
    """[R,bins,bs] taps -> float64 [R,bins,n]: the total bilinear weight a bin's samples put on each row / column."""
    R, nbin, bs = valid.shape
    w = np.zeros((R, nbin, n))
    fr = frac.astype(f64)
    r = np.arange(R)[:, None, None]
    b = np.arange(nbin)[None, :, None]
    np.add.at(w, (r, b, i0), np.where(valid, 1.0 - fr, 0.0))
    np.add.at(w, (r, b, i1), np.where(valid, fr, 0.0))
    return w


def psroi_bwd(dout, fmap_shape, boxes, box_ind, crop, bins):
    """Gradient of psroi with respect to the score map: pixel (y,x) of channel g*Cc+c receives, from every RoI r of its
    image, dout[r,c] / count * wy[r,by,y] * wx[r,bx,x], the bilinear weights factoring into a row and a column sum.
    -> (grad, n, sabs) [B,H,W,nb*Cc]: sum, number of RoIs contributing a non-zero term, sum of |term|."""
    B, H, W, Ct = fmap_shape
    nb = bins[0] * bins[1]
    Cc = Ct // nb
    bs = (crop[0] // bins[0], crop[1] // bins[1])
    boxes = np.asarray(boxes, f32)
    box_ind = np.asarray(box_ind, np.int64)
    wy = _axis_weights(*psroi_axis(boxes[:, 0], boxes[:, 2], H, bins[0], bs[0]), H)
    wx = _axis_weights(*psroi_axis(boxes[:, 1], boxes[:, 3], W, bins[1], bs[1]), W)
    d = dout.astype(f64) / (nb * bs[0] * bs[1])
    grad, n, sabs = np.zeros(fmap_shape), np.zeros(fmap_shape, np.int64), np.zeros(fmap_shape)
    for img in range(B):
        rr = np.nonzero(box_ind == img)[0]
        if not len(rr):
            continue
        for b0 in range(bins[0]):
            for b1 in range(bins[1]):
                gsl = slice((b0 * bins[1] + b1) * Cc, (b0 * bins[1] + b1 + 1) * Cc)
                w = (wy[rr, b0][:, :, None] * wx[rr, b1][:, None, :]).reshape(len(rr), H * W)
                grad[img, :, :, gsl] = (w.T @ d[rr]).reshape(H, W, Cc)
                sabs[img, :, :, gsl] = (w.T @ np.abs(d[rr])).reshape(H, W, Cc)
                n[img, :, :, gsl] = np.rint((w != 0).astype(f64).T @ (d[rr] != 0).astype(f64)).reshape(H, W, Cc)
    return grad, n, sabs


# ------------------------------------------------------------------------------------------------ bilinear resize
def resize_axis(n, on):
    """tf.image.resize_images(BILINEAR, align_corners=False), TF 1.7 resize_bilinear_op.cc (call site
    faster_rcnn_meta_arch.py:1870-1871) along one axis, in float32: s = float32(n / on); f = float32(o) * s;
    i0 = floor(f); i1 = min(i0 + 1, n - 1); l = f - i0."""
    s = f32(n) / f32(on)
    f = np.arange(on, dtype=f32) * s
    assert f.dtype == f32
    i0 = np.floor(f).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    frac = f - i0.astype(f32)
    assert frac.dtype == f32
    return i0, i1, frac


def resize_bilinear(x, OH, OW):
    """x float32 [N,H,W,C] -> (val float64 [N,OH,OW,C], amax = max |corner| per element)."""
    N, H, W, C = x.shape
    y0, y1, yl = resize_axis(H, OH)
    x0, x1, xl = resize_axis(W, OW)
    xd = x.astype(f64)
    tl, tr = xd[:, y0][:, :, x0], xd[:, y0][:, :, x1]
    bl, br = xd[:, y1][:, :, x0], xd[:, y1][:, :, x1]
    xw, yw = xl.astype(f64)[None, None, :, None], yl.astype(f64)[None, :, None, None]
    top = tl + (tr - tl) * xw
    bot = bl + (br - bl) * xw
    return top + (bot - top) * yw, np.maximum(np.maximum(np.abs(tl), np.abs(tr)), np.maximum(np.abs(bl), np.abs(br)))


def resize_bilinear_bwd(dy, in_shape):
    """Adjoint of resize_bilinear (resize_bilinear_op.cc ResizeBilinearGrad): every output pixel sends
    g*(1-yl)*(1-xl), g*(1-yl)*xl, g*yl*(1-xl), g*yl*xl to (y0,x0), (y0,x1), (y1,x0), (y1,x1).
    -> (grad, n, sabs) [N,H,W,C]; n counts every corner that lands on the element (zero weights included: the kernel's
    gather adds them too)."""
    N, H, W, C = in_shape
    OH, OW = dy.shape[1], dy.shape[2]
    y0, y1, yl = resize_axis(H, OH)
    x0, x1, xl = resize_axis(W, OW)
    g = dy.astype(f64)
    grad, n, sabs = np.zeros(in_shape), np.zeros(in_shape, np.int64), np.zeros(in_shape)
    ylw, xlw = yl.astype(f64), xl.astype(f64)
    for yy, wy in ((y0, 1.0 - ylw), (y1, ylw)):
        for xx, wx in ((x0, 1.0 - xlw), (x1, xlw)):
            c = g * wy[None, :, None, None] * wx[None, None, :, None]
            idx = (slice(None), yy[:, None], xx[None, :])
            np.add.at(grad, idx, c)
            np.add.at(sabs, idx, np.abs(c))
            np.add.at(n, idx, 1)
    return grad, n, sabs


# ------------------------------------------------------------------------------------------------------- pooling
def _padded(x, k, stride, pt, pl, OH, OW, fill):
    N, H, W, C = x.shape
    PH, PW = max((OH - 1) * stride + k, H + pt), max((OW - 1) * stride + k, W + pl)
    xp = np.full((N, PH, PW, C), fill, x.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp


def _win(a, d0, d1, stride, OH, OW):
    return a[:, d0:d0 + (OH - 1) * stride + 1:stride, d1:d1 + (OW - 1) * stride + 1:stride]


def max_pool(x, k, stride, padding):
    """slim.max_pool2d (TF MaxPool; padded cells never win). Exact in any precision: returns x's dtype."""
    pt, pl, OH, OW = pool_geometry(x.shape[1], x.shape[2], k, stride, padding)
    xp = _padded(x, k, stride, pt, pl, OH, OW, -np.inf)
    y = np.full((x.shape[0], OH, OW, x.shape[3]), -np.inf, x.dtype)
    for d in range(k * k):
        y = np.maximum(y, _win(xp, d // k, d % k, stride, OH, OW))
    return y


def max_pool_bwd(x, dy, k, stride, padding):
    """TF MaxPoolGrad: each window's gradient goes to its FIRST maximum in (dy, dx) window order.
    -> (grad, n, sabs) shaped like x: an element can be the first maximum of several overlapping windows."""
    N, H, W, C = x.shape
    pt, pl, OH, OW = pool_geometry(H, W, k, stride, padding)
    xp = _padded(x, k, stride, pt, pl, OH, OW, -np.inf)
    y = max_pool(x, k, stride, padding)
    g = dy.astype(f64)
    grad, n, sabs = np.zeros(xp.shape), np.zeros(xp.shape, np.int64), np.zeros(xp.shape)
    taken = np.zeros(y.shape, bool)
    for d in range(k * k):
        hit = (_win(xp, d // k, d % k, stride, OH, OW) == y) & ~taken
        taken |= hit
        _win(grad, d // k, d % k, stride, OH, OW)[...] += np.where(hit, g, 0.0)
        _win(sabs, d // k, d % k, stride, OH, OW)[...] += np.where(hit, np.abs(g), 0.0)
        _win(n, d // k, d % k, stride, OH, OW)[...] += hit
    assert taken.all()
    c = (slice(None), slice(pt, pt + H), slice(pl, pl + W))
    return grad[c], n[c], sabs[c]


def avg_pool(x, k, stride, padding):
    """slim.avg_pool2d (TF AvgPool: the divisor is the number of IN-BOUNDS cells of the window).
    -> (val float64, cnt int64 [OH,OW], sabs = sum |x| over the window)."""
    N, H, W, C = x.shape
    pt, pl, OH, OW = pool_geometry(H, W, k, stride, padding)
    xp = _padded(x.astype(f64), k, stride, pt, pl, OH, OW, 0.0)
    op = _padded(np.ones((1, H, W, 1)), k, stride, pt, pl, OH, OW, 0.0)
    s, sabs, cnt = 0.0, 0.0, 0.0
    for d in range(k * k):
        s = s + _win(xp, d // k, d % k, stride, OH, OW)
        sabs = sabs + np.abs(_win(xp, d // k, d % k, stride, OH, OW))
        cnt = cnt + _win(op, d // k, d % k, stride, OH, OW)
    return s / cnt, cnt[0, :, :, 0].astype(np.int64), sabs


def avg_pool_bwd(dy, x_shape, k, stride, padding):
    """TF AvgPoolGrad: dx = sum over the windows covering the cell of dy / count(window). -> (grad, n, sabs)."""
    N, H, W, C = x_shape
    pt, pl, OH, OW = pool_geometry(H, W, k, stride, padding)
    _, cnt, _ = avg_pool(np.zeros((1, H, W, 1), f32), k, stride, padding)
    t = dy.astype(f64) / cnt[None, :, :, None]
    shape = _padded(np.zeros(x_shape, f32), k, stride, pt, pl, OH, OW, 0.0).shape
    grad, n, sabs = np.zeros(shape), np.zeros(shape, np.int64), np.zeros(shape)
    for d in range(k * k):
        _win(grad, d // k, d % k, stride, OH, OW)[...] += t
        _win(sabs, d // k, d % k, stride, OH, OW)[...] += np.abs(t)
        _win(n, d // k, d % k, stride, OH, OW)[...] += 1
    c = (slice(None), slice(pt, pt + H), slice(pl, pl + W))
    return grad[c], n[c], sabs[c]


# ----------------------------------------------------------------------------------------------------- depthwise
def _dw_geometry(H, W, stride, dilation):
    pt, OH = same_pad(H, 3, stride, dilation)
    pl, OW = same_pad(W, 3, stride, dilation)
    return pt, pl, OH, OW


def _dw_win(a, r, s, stride, dilation, OH, OW):
    return a[:, r * dilation:r * dilation + (OH - 1) * stride + 1:stride,
             s * dilation:s * dilation + (OW - 1) * stride + 1:stride]


def _dw_pad(x, stride, dilation):
    N, H, W, C = x.shape
    pt, pl, OH, OW = _dw_geometry(H, W, stride, dilation)
    PH = max((OH - 1) * stride + 2 * dilation + 1, H + pt)
    PW = max((OW - 1) * stride + 2 * dilation + 1, W + pl)
    xp = np.zeros((N, PH, PW, C), f64)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp, pt, pl, OH, OW


def depthwise(x, w, stride=1, dilation=1, bias=None):
    """tf.nn.depthwise_conv2d, 3x3, SAME, multiplier 1 (slim.separable_conv2d's depthwise stage,
    slim/nets/mobilenet_v1.py:229-245). x [N,H,W,C], w [3,3,C]. -> (pre-activation float64, sabs = sum |x*w| (+|bias|))."""
    xp, pt, pl, OH, OW = _dw_pad(x, stride, dilation)
    wd = w.astype(f64)
    y, sabs = 0.0, 0.0
    for r in range(3):
        for s in range(3):
            t = _dw_win(xp, r, s, stride, dilation, OH, OW) * wd[r, s]
            y, sabs = y + t, sabs + np.abs(t)
    if bias is not None:
        y, sabs = y + bias.astype(f64), sabs + np.abs(bias.astype(f64))
    return y, sabs


def depthwise_dgrad(g, w, x_shape, stride=1, dilation=1):
    """DepthwiseConv2dNativeBackpropInput: dx = sum over taps of g[(ih+pt-r*dil)/stride, ...] * w[r,s]. -> (grad, sabs)."""
    N, H, W, C = x_shape
    xp, pt, pl, OH, OW = _dw_pad(np.zeros(x_shape, f32), stride, dilation)
    grad, sabs = np.zeros(xp.shape), np.zeros(xp.shape)
    gd, wd = g.astype(f64), w.astype(f64)
    for r in range(3):
        for s in range(3):
            t = gd * wd[r, s]
            _dw_win(grad, r, s, stride, dilation, OH, OW)[...] += t
            _dw_win(sabs, r, s, stride, dilation, OH, OW)[...] += np.abs(t)
    c = (slice(None), slice(pt, pt + H), slice(pl, pl + W))
    return grad[c], sabs[c]


def depthwise_wgrad(x, g, stride=1, dilation=1):
    """DepthwiseConv2dNativeBackpropFilter: dw[r,s,c] = sum over output pixels of x[tap] * g. -> (dw, sabs) [3,3,C]."""
    xp, pt, pl, OH, OW = _dw_pad(x, stride, dilation)
    gd = g.astype(f64)
    C = x.shape[3]
    dw, sabs = np.zeros((3, 3, C)), np.zeros((3, 3, C))
    for r in range(3):
        for s in range(3):
            t = _dw_win(xp, r, s, stride, dilation, OH, OW) * gd
            dw[r, s], sabs[r, s] = t.sum((0, 1, 2)), np.abs(t).sum((0, 1, 2))
    return dw, sabs


# ---------------------------------------------------------------------------------- BatchNorm parameter gradients
def bn_param_grads(y, g, gamma, beta):
    """Gradients of the trainable gamma / beta of slim.batch_norm(is_training=False) folded into the producing layer:
    y = gamma * xhat + beta wherever g != 0, so dbeta = sum g, dgamma = sum g * xhat = sum g * (y - beta) / gamma;
    a gamma of exactly 0 is reported as 0 (xhat cannot be recovered). y, g [rows,C].
    -> (dgamma, dbeta, s_gy = sum |g*(y-beta)|, s_g = sum |g|), float64 [C]."""
    yd, gd, bd, gm = y.astype(f64), g.astype(f64), beta.astype(f64), gamma.astype(f64)
    t = gd * (yd - bd)
    nz = gm != 0
    dgamma = np.where(nz, t.sum(0) / np.where(nz, gm, 1.0), 0.0)
    return dgamma, gd.sum(0), np.abs(t).sum(0), np.abs(gd).sum(0)


# -------------------------------------------------------------------------------------------------- spatial mean
def spatial_mean(x):
    """tf.reduce_mean(x, [1, 2]) (core/box_predictor.py:471: the average of the second-stage tower's output). -> (mean, sum |x|)."""
    xd = x.astype(f64)
    return xd.mean((1, 2)), np.abs(xd).sum((1, 2))


def spatial_mean_bwd(dy, shape, act=None, relu6=False):
    """dx = dy / HW broadcast over the pixels; with `act`, times the ReLU (0 < act) or ReLU6 (0 < act < 6) gradient
    of the averaged activation (tf.nn.relu / relu6 gradients are zero AT the clipping points)."""
    N, H, W, C = shape
    dx = np.broadcast_to((dy.astype(f64) / (H * W))[:, None, None, :], shape)
    if act is None:
        return dx.copy()
    on = (act > 0) & ((act < 6) if relu6 else True)
    return np.where(on, dx, 0.0)


# ------------------------------------------------------------------------------------------------ box utilities
def expand_windows_f32(prop, n_expand):
    """faster_rcnn_meta_arch.py:776-803 in float32, operation by operation: window i = the proposal pushed i/(n-1) of
    the way to the full image: [y1 - y1/(n-1)*i, x1 - x1/(n-1)*i, y2 + (1-y2)/(n-1)*i, x2 + (1-x2)/(n-1)*i].
    prop float32 [B,n2,4] -> float32 [B,n_expand,n2,4]."""
    p = np.asarray(prop, f32)
    ne = f32(n_expand - 1)
    d = np.stack([p[..., 0] / ne, p[..., 1] / ne, (f32(1) - p[..., 2]) / ne, (f32(1) - p[..., 3]) / ne], -1)
    sign = np.array([-1, -1, 1, 1], f32)
    out = np.stack([p + sign * (d * f32(i)) for i in range(n_expand)], 1)
    assert out.dtype == f32
    return out


def expand_windows(prop, n_expand):
    """The same in float64 (exact inputs, unrounded arithmetic)."""
    p = np.asarray(prop, f32).astype(f64)
    d = np.stack([p[..., 0], p[..., 1], 1.0 - p[..., 2], 1.0 - p[..., 3]], -1) / (n_expand - 1)
    sign = np.array([-1.0, -1.0, 1.0, 1.0])
    return np.stack([p + sign * d * i for i in range(n_expand)], 1)


def clip_to_window(boxes, window):
    """box_list_ops.clip_to_window (core/box_list_ops.py:102-134) without the empty-box filter:
    maximum(minimum(v, win_max), win_min) per coordinate."""
    b = np.asarray(boxes, f32)
    w = np.asarray(window, f32)
    lo = np.array([w[0], w[1], w[0], w[1]], f32)
    hi = np.array([w[2], w[3], w[2], w[3]], f32)
    return np.maximum(np.minimum(b, hi), lo)
