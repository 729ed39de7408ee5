"""Training-time data augmentation: every one of the reference's pipeline configs
enables exactly `random_horizontal_flip`; a config may also list the options that only touch pixels.

Restates core/preprocessor.py:145-168 (flip_boxes) and :239-345 (random_horizontal_flip with the
fork's extra window boxes and edge masks) on host numpy arrays — the input pipeline is host-side in
the reference too (queue runners feeding the graph, trainer.py:47-98) — and the photometric options
(normalize_image :120, subtract_channel_mean :1490, random_adjust_brightness / contrast / hue /
saturation :459-540, random_distort_color :542, random_rgb_to_gray :430, random_pixel_value_scale :347,
random_black_patches :1189) plus random_jitter_boxes :578 as an op program (see OP_* below). This host
restatement is the feed of the host generator and the yardstick of the device kernel
(csrc/ops.hip k_prepare_images_aug), the role resize_bilinear_legacy plays for the resize.

Randomness: every option takes a fixed number of uniform draws from the consumer's RandomState, so the
asynchronous pipeline can replay them without decoding; per-element (pixel scale) and per-box (jitter)
uniforms come from the samplers' counter hash mix32 seeded by the option's one draw. The hue and saturation
ops restate TF 1.7's CPU kernels (adjust_hue_op.cc, adjust_saturation_op.cc) as fixed float32 sequences;
TensorFlow cannot run here, so the restatement is pinned by tests against Python's colorsys (float64) and by
known answers, not by TF output. The contrast mean sums in float64 in a fixed order (contrast_mean), where
TF's Eigen reduction order is unspecified. core/preprocessor.py:1989 prevent_box_size_zero, which the
reference runs after an augmented preprocess, is not applied (it would change flip-only configs).
"""
import numpy as np


def flip_boxes(boxes):
    """Left-right flip of normalised [ymin, xmin, ymax, xmax] boxes: xmin' = 1 - xmax, xmax' = 1 - xmin."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    one = np.float32(1.0)
    return np.stack([b[:, 0], one - b[:, 3], b[:, 2], one - b[:, 1]], 1)


def random_horizontal_flip(image, boxes, window_boxes=None, edgemask=None, rng=None, do_flip=None,
                           reference_edgemask_axis=True):
    """image [H,W,3]; boxes [N,4] normalised; window_boxes [Wn,4]; edgemask [2,h,w] (fg, weight).

    The flip happens with probability 0.5 (`uniform > 0.5`) and only if the image has boxes
    (preprocessor.py:300-304). The reference passes the [2,h,w] edge mask to
    tf.image.flip_left_right, which treats it as [height=2, width=h, channels=w] and therefore
    reverses the mask ROWS, not its columns (:340-342); `reference_edgemask_axis=True` reproduces
    that, False mirrors the columns like the image."""
    image = np.asarray(image)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    if do_flip is None:
        rng = rng if rng is not None else np.random
        do_flip = float(rng.uniform()) > 0.5
    do_flip = bool(do_flip) and boxes.size > 0
    out = [image[:, ::-1].copy() if do_flip else image, flip_boxes(boxes) if do_flip else boxes]
    if window_boxes is not None:
        wb = np.asarray(window_boxes, np.float32).reshape(-1, 4)
        out.append(flip_boxes(wb) if do_flip else wb)
    if edgemask is not None:
        em = np.asarray(edgemask)
        if do_flip:
            em = em[:, ::-1].copy() if reference_edgemask_axis else em[:, :, ::-1].copy()
        out.append(em)
    return tuple(out)


# ------------------------------------------------------------------------------ photometric augmentation
# The options that only touch pixels (and random_jitter_boxes, which only touches groundtruth_boxes): the only ones
# sound with the fork's multi-task labels. core/preprocessor.py:1812-1903 get_default_func_arg_map hands them `image`
# alone (jitter: `groundtruth_boxes` alone), so window boxes / labels, closeness and the edge mask stay valid.
# Each option becomes a short list of primitive ops; the PROGRAM (op codes) is the same for every image of a config,
# the PARAMETERS (float32, computed here from the consumer's uniform draws and the image size) differ per image.
# apply_program evaluates them on the host; csrc/ops.hip k_prepare_images_aug evaluates the same float32 sequence
# on the device (before the resize), so the two agree to the bit.
OP_FLIP, OP_NORMALIZE, OP_SUB_MEAN, OP_ADD, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_CLIP, OP_GRAY, OP_PIXEL_SCALE, \
    OP_PATCH = range(11)
OP_PARAMS = (1, 3, 3, 1, 1, 1, 1, 0, 1, 3, 4)      # float32 parameters per op, in op order (csrc/ops.hip aug_nparams)
PIXEL_SCALE_STREAM = 0x50584C53                    # mix32 stream of random_pixel_value_scale
JITTER_STREAM = 0x4A495452                         # mix32 stream of random_jitter_boxes

# option -> config.DEFAULTS kind of its message (proto defaults; the reference's function defaults are the same)
OPTION_KIND = {
    "random_horizontal_flip": "RandomHorizontalFlip", "normalize_image": "NormalizeImage",
    "subtract_channel_mean": "SubtractChannelMean", "random_adjust_brightness": "RandomAdjustBrightness",
    "random_adjust_contrast": "RandomAdjustContrast", "random_adjust_saturation": "RandomAdjustSaturation",
    "random_adjust_hue": "RandomAdjustHue", "random_distort_color": "RandomDistortColor",
    "random_rgb_to_gray": "RandomRGBtoGray", "random_pixel_value_scale": "RandomPixelValueScale",
    "random_black_patches": "RandomBlackPatches", "random_jitter_boxes": "RandomJitterBoxes",
}
_GEOMETRIC = ("random_crop_image", "random_pad_image", "random_crop_pad_image", "random_crop_to_aspect_ratio",
              "ssd_random_crop", "ssd_random_crop_pad", "ssd_random_crop_fixed_aspect_ratio")
_RESIZING = ("random_image_scale", "random_resize_method", "resize_image")
_CLIPPING = ("random_adjust_brightness", "random_adjust_contrast", "random_adjust_saturation", "random_adjust_hue",
             "random_distort_color", "random_pixel_value_scale")
_warned_range = False


def refusal(kind):
    """The error of an option this path does not run."""
    if kind in _GEOMETRIC:
        why = ("it moves groundtruth_boxes / classes but would leave the window boxes, closeness labels and edge mask "
               "of the multi-task heads in the old frame")
    elif kind in _RESIZING:
        why = "it resizes the image, which composes with the model's resize_to_range image resizer"
    elif kind == "scale_boxes_to_pixel_coordinates":
        why = "the model's losses and targets take normalised boxes"
    else:
        why = "it is no PreprocessingStep option of the reference this path implements (%s)" % ", ".join(
            sorted(OPTION_KIND))
    return ValueError("data augmentation %r is not supported: %s" % (kind, why))


class Step:
    """One parsed data_augmentation_options entry: `kind` and its arguments with the proto defaults filled in."""

    def __init__(self, kind, args):
        self.kind, self.args = kind, args

    def __repr__(self):
        return "Step(%r, %r)" % (self.kind, self.args)

    @property
    def draws(self):
        """Uniform draws per example: fixed, whatever the pixels or the boxes."""
        k = self.kind
        if k in ("normalize_image", "subtract_channel_mean"):
            return 0
        if k == "random_distort_color":
            return 4
        if k == "random_black_patches":
            return 3 * int(self.args["max_black_patches"])
        return 1


def _entries(options):
    for opt in options:
        if hasattr(opt, "keys"):
            for kind in opt.keys():
                yield kind, opt[kind]
        else:
            yield opt, None


def parse_options(options, warn=True):
    """data_augmentation_options (parsed config messages, {kind: {field: value}} dicts or bare option names) ->
    [Step], in config order. Refuses what this path does not run; logs once when an option that clips to [0, 1]
    runs on pixels that no earlier normalize_image mapped to [0, 1] (the reference's own trap: pixels are 0..255
    there, trainer.py:70-73, so such an option alone saturates almost every pixel)."""
    from . import config
    global _warned_range
    steps, unit = [], False
    for kind, val in _entries(options or ()):
        if kind not in OPTION_KIND:
            raise refusal(kind)
        defaults = config.DEFAULTS[OPTION_KIND[kind]]
        val = val or {}
        args = {f: (list(val[f]) if f == "means" else val[f]) if f in val else d for f, d in defaults.items()}
        unknown = set(val) - set(defaults)
        if unknown:
            raise ValueError("%s has no field(s) %s" % (kind, sorted(unknown)))
        if kind == "normalize_image":
            if float(args["original_maxval"]) == float(args["original_minval"]):
                raise ValueError("normalize_image needs original_maxval != original_minval")
            unit = float(args["target_minval"]) == 0.0 and float(args["target_maxval"]) == 1.0
        elif kind == "subtract_channel_mean" and len(args["means"]) != 3:
            raise ValueError("subtract_channel_mean: len(means) must match the number of channels (3)")
        elif kind == "random_distort_color" and int(args["color_ordering"]) not in (0, 1):
            raise ValueError("random_distort_color: color_ordering must be in {0, 1}")
        elif kind == "random_adjust_hue" and not 0.0 <= float(args["max_delta"]) <= 0.5:
            raise ValueError("random_adjust_hue: max_delta must be in [0, 0.5]")
        if kind in _CLIPPING and not unit and warn and not _warned_range:
            _warned_range = True
            import logging
            logging.getLogger(__name__).warning(
                "%s clips to [0, 1] but no earlier normalize_image maps the 0..255 pixels to [0, 1]: almost every "
                "pixel saturates, as in the reference. List normalize_image (0..255 -> 0..1) before the colour "
                "options and normalize_image (0..1 -> 0..255) after them.", kind)
        steps.append(Step(kind, args))
    return steps


def draw_count(steps):
    return sum(s.draws for s in steps)


# random_distort_color (:542-575): the four steps of each ordering and the ranges of their draws
_DISTORT = {0: (OP_ADD, OP_SATURATION, OP_HUE, OP_CONTRAST), 1: (OP_ADD, OP_CONTRAST, OP_SATURATION, OP_HUE)}
_DISTORT_RANGE = {OP_ADD: (-32.0 / 255.0, 32.0 / 255.0), OP_SATURATION: (0.5, 1.5), OP_HUE: (-0.2, 0.2),
                  OP_CONTRAST: (0.5, 1.5)}


def program(steps):
    """The op codes of a parsed option list (the same for every image)."""
    codes = []
    for s in steps:
        k = s.kind
        if k == "random_horizontal_flip":
            codes.append(OP_FLIP)
        elif k == "normalize_image":
            codes.append(OP_NORMALIZE)
        elif k == "subtract_channel_mean":
            codes.append(OP_SUB_MEAN)
        elif k == "random_adjust_brightness":
            codes += [OP_ADD, OP_CLIP]
        elif k == "random_adjust_contrast":
            codes += [OP_CONTRAST, OP_CLIP]
        elif k == "random_adjust_saturation":
            codes += [OP_SATURATION, OP_CLIP]
        elif k == "random_adjust_hue":
            codes += [OP_HUE, OP_CLIP]
        elif k == "random_distort_color":              # no clip between the four steps (:542-575)
            codes += list(_DISTORT[int(s.args["color_ordering"])]) + [OP_CLIP]
        elif k == "random_rgb_to_gray":
            codes.append(OP_GRAY)
        elif k == "random_pixel_value_scale":
            codes += [OP_PIXEL_SCALE, OP_CLIP]
        elif k == "random_black_patches":
            codes += [OP_PATCH] * int(s.args["max_black_patches"])
    return codes


def num_params(codes):
    return sum(OP_PARAMS[c] for c in codes)


def _uniform(u, lo, hi):
    """tf.random_uniform([], lo, hi) from one draw u in [0, 1): lo + (hi - lo) * u in double, rounded once."""
    return np.float32(float(lo) + (float(hi) - float(lo)) * float(u))


def _seed(u):
    return int(float(u) * 4294967296.0) & 0xFFFFFFFF


def plan(steps, draws, H, W, num_boxes):
    """-> (float32 [num_params(program(steps))] parameters of one H x W image, label actions). The draws are the
    consumer's uniform draws of the example, draw_count(steps) of them, in option order. Label actions, in config
    order: ("flip", flag) and ("jitter", seed, ratio)."""
    draws = [float(u) for u in draws]
    if len(draws) != draw_count(steps):
        raise ValueError("%d draws for options that take %d" % (len(draws), draw_count(steps)))
    it = iter(draws)
    p, actions = [], []
    for s in steps:
        k, a = s.kind, s.args
        if k == "random_horizontal_flip":
            # one draw per listed option, boxes or not; an image without boxes is never flipped (:300-304)
            flag = next(it) > 0.5 and num_boxes > 0
            p.append(1.0 if flag else 0.0)
            actions.append(("flip", flag))
        elif k == "normalize_image":
            omin, omax = float(a["original_minval"]), float(a["original_maxval"])
            tmin, tmax = float(a["target_minval"]), float(a["target_maxval"])
            p += [np.float32(omin), np.float32((tmax - tmin) / (omax - omin)), np.float32(tmin)]
        elif k == "subtract_channel_mean":
            p += [np.float32(m) for m in a["means"]]
        elif k == "random_adjust_brightness":
            p.append(_uniform(next(it), -float(a["max_delta"]), float(a["max_delta"])))
        elif k in ("random_adjust_contrast", "random_adjust_saturation"):
            p.append(_uniform(next(it), a["min_delta"], a["max_delta"]))
        elif k == "random_adjust_hue":
            p.append(_uniform(next(it), -float(a["max_delta"]), float(a["max_delta"])))
        elif k == "random_distort_color":
            for code in _DISTORT[int(a["color_ordering"])]:
                p.append(_uniform(next(it), *_DISTORT_RANGE[code]))
        elif k == "random_rgb_to_gray":
            p.append(1.0 if next(it) <= float(a["probability"]) else 0.0)     # gray unless u > probability
        elif k == "random_pixel_value_scale":
            lo, hi = float(a["minval"]), float(a["maxval"])
            p += [np.uint32(_seed(next(it))).view(np.float32), np.float32(lo), np.float32(hi - lo)]
        elif k == "random_black_patches":
            ratio = np.float32(a["size_to_image_ratio"])
            box = int(np.float32(min(H, W)) * ratio)
            span = np.float32(1.0 - float(a["size_to_image_ratio"]))
            for _ in range(int(a["max_black_patches"])):
                up, uy, ux = next(it), next(it), next(it)
                y0 = int((np.float32(uy) * span) * np.float32(H))
                x0 = int((np.float32(ux) * span) * np.float32(W))
                p += [1.0 if up <= float(a["probability"]) else 0.0, float(y0), float(x0), float(box)]
        elif k == "random_jitter_boxes":
            actions.append(("jitter", _seed(next(it)), float(a["ratio"])))
    return np.array(p, np.float32), actions


def mix32(seed, stream, i):
    """The samplers' counter hash (csrc/glue.hip glue_mix32) on uint32 arrays."""
    m = 0xFFFFFFFF
    x = (np.asarray(i, np.uint64) + (0x9E3779B9 * int(seed) + 0x85EBCA6B * int(stream))) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def hash_uniform(seed, stream, i):
    """float32 in [0, 1) of element i: (mix32 >> 8) * 2^-24, exact in float32 (device: aug_uniform)."""
    return (mix32(seed, stream, i) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def jitter_boxes(boxes, seed, ratio):
    """core/preprocessor.py:578-625 random_jitter_boxes: each corner += U[-ratio, ratio) * (box height or width),
    clipped to [0, 1]; the uniform of coordinate j of box n is hash_uniform(seed, JITTER_STREAM, 4 n + j)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    u = hash_uniform(seed, JITTER_STREAM, np.arange(b.size, dtype=np.uint64)).reshape(-1, 4)
    r = np.float32(-ratio) + np.float32(2.0 * ratio) * u
    h, w = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    hw = np.stack([h, w, h, w], 1)
    return np.minimum(np.maximum(b + hw * r, np.float32(0)), np.float32(1))


def contrast_mean(x):
    """Per-channel mean of a float32 [H,W,3] image for adjust_contrast: float64 sums, x ascending within a row, then
    the row sums ascending, divided by H*W and rounded once to float32 (the device pre-pass k_aug_rowsum /
    k_aug_mean adds in the same order). np.cumsum adds sequentially; np.sum would add pairwise."""
    H, W = x.shape[:2]
    rows = np.cumsum(np.asarray(x, np.float64), axis=1)[:, -1, :]
    return (np.cumsum(rows, axis=0)[-1] / float(H * W)).astype(np.float32)


_F = np.float32


def rgb_to_hv_range(r, g, b):
    """TF 1.7 adjust_hue_op.cc rgb_to_hv_range on float32 arrays: (h in [0, 6], v_min, v_max)."""
    rg = r < g
    vmax = np.where(rg, np.where(b < r, g, np.where(b > g, b, g)), np.where(b < g, r, np.where(b > r, b, r)))
    vmid = np.where(rg, np.where(b < r, r, np.where(b > g, g, b)), np.where(b < g, g, np.where(b > r, r, b)))
    vmin = np.where(rg, np.where(b < r, b, r), np.where(b < g, b, g))
    cat = np.where(rg, np.where(b < r, 1, np.where(b > g, 3, 2)), np.where(b < g, 0, np.where(b > r, 4, 5)))
    with np.errstate(all="ignore"):
        ratio = (vmid - vmin) / (vmax - vmin)
        h = cat.astype(_F) + np.where(cat % 2 == 0, ratio, _F(1) - ratio)
    return np.where(vmax == vmin, _F(0), h).astype(_F), vmin, vmax


def hv_range_to_rgb(h, vmin, vmax):
    """TF 1.7 adjust_hue_op.cc hv_range_to_rgb."""
    cat = h.astype(np.int32)
    ratio = h - cat.astype(_F)
    ratio = np.where(cat % 2 == 1, _F(1) - ratio, ratio)
    vmid = vmin + ratio * (vmax - vmin)
    table = [(vmax, vmid, vmin), (vmid, vmax, vmin), (vmin, vmax, vmid), (vmin, vmid, vmax), (vmid, vmin, vmax)]
    out = [vmax, vmin, vmid]                               # case 5 and default
    for c in range(4, -1, -1):
        out = [np.where(cat == c, t, o) for t, o in zip(table[c], out)]
    return out


def adjust_hue(r, g, b, delta):
    """TF 1.7 AdjustHueOp: rotate the hue by delta * 6 with the kernel's `while` wraps into [0, 6)."""
    h, vmin, vmax = rgb_to_hv_range(r, g, b)
    h = h + _F(delta) * _F(6)
    while (h < 0).any():
        h = np.where(h < 0, h + _F(6), h)
    while (h >= 6).any():
        h = np.where(h >= 6, h - _F(6), h)
    return hv_range_to_rgb(h, vmin, vmax)


def rgb_to_hsv(r, g, b):
    """TF 1.7 adjust_saturation_op.cc rgb_to_hsv; the 2/6 and 4/6 offsets are double constants there."""
    vv = np.maximum(r, np.maximum(g, b))
    rng = vv - np.minimum(r, np.minimum(g, b))
    with np.errstate(all="ignore"):
        s = np.where(vv > 0, rng / vv, _F(0)).astype(_F)
        norm = _F(1) / (_F(6) * rng)
        hr = norm * (g - b)
        hg = ((norm * (b - r)).astype(np.float64) + 2.0 / 6.0).astype(_F)
        hb = ((norm * (r - g)).astype(np.float64) + 4.0 / 6.0).astype(_F)
    hh = np.where(r == vv, hr, np.where(g == vv, hg, hb))
    hh = np.where(rng <= 0, _F(0), hh)
    hh = np.where(hh < 0, hh + _F(1), hh)
    return hh.astype(_F), s, vv


def hsv_to_rgb(h, s, v):
    """TF 1.7 adjust_saturation_op.cc hsv_to_rgb (its `while` wraps, not fmod)."""
    c = s * v
    m = v - c
    dh = h * _F(6)
    cat = dh.astype(np.int32)
    f = dh
    while (f <= 0).any():
        f = np.where(f <= 0, f + _F(2), f)
    while (f >= 2).any():
        f = np.where(f >= 2, f - _F(2), f)
    x = c * (_F(1) - np.abs(f - _F(1)))
    z = np.zeros_like(c)
    table = [(c, x, z), (x, c, z), (z, c, x), (z, x, c), (x, z, c), (c, z, x)]
    out = [z, z, z]                                        # default (h * 6 == 6)
    for k in range(5, -1, -1):
        out = [np.where(cat == k, t, o) for t, o in zip(table[k], out)]
    return [o + m for o in out]


def adjust_saturation(r, g, b, k):
    """TF 1.7 AdjustSaturationOp: s = min(1, max(0, s * k)) in HSV."""
    h, s, v = rgb_to_hsv(r, g, b)
    s = np.minimum(_F(1), np.maximum(_F(0), s * _F(k)))
    return hsv_to_rgb(h, s, v)


def apply_program(image, codes, params):
    """The primitive ops `codes` with one image's `params` on an [H,W,3] image (config order, at its own size). A
    flip mirrors whatever dtype it gets (the flip-only path is unchanged); every other op works on float32 (0..255
    from the decoder, or whatever earlier ops made of it). Position-dependent ops (black patches, the per-element
    pixel scale, the contrast mean) use the image as it is at that stage."""
    x = np.asarray(image)
    params = np.asarray(params, np.float32)
    H, W = x.shape[:2]
    k = 0
    for code in codes:
        p = params[k:k + OP_PARAMS[code]]
        k += OP_PARAMS[code]
        if code == OP_FLIP:
            if p[0] != 0:
                x = x[:, ::-1].copy()
            continue
        x = np.asarray(x, np.float32)
        if code == OP_NORMALIZE:
            x = (x - p[0]) * p[1] + p[2]
        elif code == OP_SUB_MEAN:
            x = x - p[None, None, :]
        elif code == OP_ADD:
            x = x + p[0]
        elif code == OP_CONTRAST:
            m = contrast_mean(x)
            x = (x - m) * p[0] + m
        elif code in (OP_SATURATION, OP_HUE):
            fn = adjust_saturation if code == OP_SATURATION else adjust_hue
            x = np.stack(fn(x[..., 0], x[..., 1], x[..., 2], p[0]), -1).astype(np.float32)
        elif code == OP_CLIP:
            x = np.minimum(np.maximum(x, _F(0)), _F(1))
        elif code == OP_GRAY:
            if p[0] != 0:
                gray = (x[..., 0] * _F(0.2989) + x[..., 1] * _F(0.5870)) + x[..., 2] * _F(0.1140)
                x = np.repeat(gray[..., None], 3, -1)
        elif code == OP_PIXEL_SCALE:
            seed = int(p[:1].view(np.uint32)[0])
            u = hash_uniform(seed, PIXEL_SCALE_STREAM, np.arange(H * W * 3, dtype=np.uint64)).reshape(H, W, 3)
            x = x * (p[1] + p[2] * u)
        elif code == OP_PATCH:
            if p[0] != 0:
                y0, x0, box = int(p[1]), int(p[2]), int(p[3])
                x = x.copy()
                x[y0:y0 + box, x0:x0 + box] *= _F(0)
        else:
            raise ValueError("bad augmentation op code %r" % code)
    if k != params.size:
        raise ValueError("%d parameters for a program that takes %d" % (params.size, k))
    return x


def apply_labels(ex, actions):
    """The label side of plan()'s actions on one example dict (flips of boxes, window boxes and edge mask; box
    jitter of groundtruth_boxes only, get_default_func_arg_map)."""
    ex = dict(ex)
    for act in actions:
        if act[0] == "flip":
            res = random_horizontal_flip(_NO_IMAGE, ex["groundtruth_boxes"], ex.get("window_boxes"),
                                         ex.get("groundtruth_edgemask"), do_flip=act[1])
            ex["groundtruth_boxes"] = res[1]
            i = 2
            if ex.get("window_boxes") is not None:
                ex["window_boxes"] = res[i]
                i += 1
            if ex.get("groundtruth_edgemask") is not None:
                ex["groundtruth_edgemask"] = res[i]
        else:
            ex["groundtruth_boxes"] = jitter_boxes(ex["groundtruth_boxes"], act[1], act[2])
    return ex


_NO_IMAGE = np.zeros((0, 0, 3), np.uint8)


def preprocess(example, data_augmentation_options, rng=None):
    """core/preprocessor.py:1905-2048 `preprocess(tensor_dict, preprocess_options)` for the options that only touch
    pixels, random_jitter_boxes and random_horizontal_flip, in config order. `example`: one image's dict with the
    fields of mtl_ssl_amd.synthetic.make_batch (unbatched): image, groundtruth_boxes, window_boxes,
    groundtruth_edgemask (class / closeness labels are invariant under these options). Every option takes a fixed
    number of rng.uniform() draws (Step.draws), taken up front in option order."""
    steps = parse_options(data_augmentation_options)
    rng = rng if rng is not None else np.random
    draws = [float(rng.uniform()) for _ in range(draw_count(steps))]
    image = np.asarray(example["image"])
    params, actions = plan(steps, draws, image.shape[0], image.shape[1],
                           np.asarray(example["groundtruth_boxes"]).reshape(-1, 4).shape[0])
    ex = apply_labels(example, actions)
    ex["image"] = apply_program(image, program(steps), params)
    return ex


def resize_bilinear_legacy(image, out_h, out_w):
    """tf.image.resize_images(image, [out_h, out_w]) as the reference's resizer calls it (bilinear,
    align_corners=False, TF 1.7: src = dst * in/out without a half-pixel offset, upper neighbour clamped to
    the edge; core/preprocessor.py:1408-1411) on a host [H,W,C] float32 array — the same arithmetic as the
    device kernel mtlssl_resize_bilinear_fwd, so a batch can be resized per image on the host and stacked."""
    x = np.asarray(image, np.float32)
    H, W = x.shape[0], x.shape[1]
    if (H, W) == (out_h, out_w):
        return x
    ys = np.arange(out_h, dtype=np.float32) * np.float32(H / out_h)
    xs = np.arange(out_w, dtype=np.float32) * np.float32(W / out_w)
    y0 = np.floor(ys).astype(np.int64); y1 = np.minimum(y0 + 1, H - 1)
    x0 = np.floor(xs).astype(np.int64); x1 = np.minimum(x0 + 1, W - 1)
    yl = (ys - y0.astype(np.float32))[:, None, None]
    xl = (xs - x0.astype(np.float32))[None, :, None]
    top = x[y0][:, x0] + (x[y0][:, x1] - x[y0][:, x0]) * xl
    bot = x[y1][:, x0] + (x[y1][:, x1] - x[y1][:, x0]) * xl
    return np.ascontiguousarray(top + (bot - top) * yl, dtype=np.float32)     # fancy indexing leaves a permuted layout
