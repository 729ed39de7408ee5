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

Geometric options (opt-in: `geometric=True`): random_crop_image :757, random_pad_image :856, random_crop_pad_image
:959 and ssd_random_crop :1548 become OP_CROP / OP_PAD in the same program, so an option listed before a crop sees the
uncropped frame and one listed after a pad the padded one. They move groundtruth_boxes / classes only; the window,
closeness and edge-mask labels frozen into a record would stay in the old frame, so a geometric example drops them and
the trainer makes them from the boxes (aux_labels="generate"). The crop window is sample_crop_window below, modelled on
TF 1.7's sample_distorted_bounding_box kernel, which is not part of the reference and cannot run here: its parity with
TensorFlow is unpinned. The mean colour of a pad is contrast_mean of the frame it receives.
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
    OP_PATCH, OP_CROP, OP_PAD = range(13)
# float32 parameters per op, in op order (csrc/ops.hip aug_nparams). OP_CROP: y0, x0, h, w (integers, exact in float32;
# the identity crop is 0, 0, H, W). OP_PAD: offset y, offset x, target h, target w, colour mode (PAD_GIVEN: r, g, b
# follow; PAD_MEAN: the mean of the frame the pad receives), r, g, b.
OP_PARAMS = (1, 3, 3, 1, 1, 1, 1, 0, 1, 3, 4, 4, 8)
GEOMETRIC_OPS = (OP_CROP, OP_PAD)
PAD_GIVEN, PAD_MEAN = 0.0, 1.0
CROP_STREAM = 0x43524F50                           # mix32 stream of the crop-window sampler
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
# the options that move the frame, run only with geometric=True
GEOMETRIC_KIND = {"random_crop_image": "RandomCropImage", "random_pad_image": "RandomPadImage",
                  "random_crop_pad_image": "RandomCropPadImage", "ssd_random_crop": "SSDRandomCrop"}
AUX_FIELDS = ("window_boxes", "window_classes", "groundtruth_closeness", "groundtruth_edgemask")
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
        if kind in GEOMETRIC_KIND:
            why += ("; it runs with geometric=True, when those labels are made from the boxes at every step "
                    "(aux_labels=\"generate\", --aux_labels=generate) or no such head is switched on")
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
        if k in _GEO_DRAWS:
            return _GEO_DRAWS[k]
        if k == "random_distort_color":
            return 4
        if k == "random_black_patches":
            return 3 * int(self.args["max_black_patches"])
        return 1


# random_crop_image: keep-the-original draw + sampler seed; random_pad_image: target h, target w, offset y, offset x;
# ssd_random_crop: case index + the selected crop's two. Every draw is taken whatever the ranges or random_coef.
_GEO_DRAWS = {"random_crop_image": 2, "random_pad_image": 4, "random_crop_pad_image": 6, "ssd_random_crop": 3}
# core/preprocessor.py:1553-1557: the seven cases of ssd_random_crop when `operations` is empty
_SSD_DEFAULT_CASES = [dict(min_object_covered=c, min_aspect_ratio=0.5, max_aspect_ratio=2.0, min_area=0.1, max_area=1.0,
                           overlap_thresh=c, random_coef=0.15) for c in (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0)]


def _check_crop(kind, a):
    """The ranges a crop's arguments must lie in; the error names the field."""
    def bad(field, rule):
        return ValueError("%s: %s = %r, need %s" % (kind, field, a[field], rule))
    if not 0.0 < float(a["min_area"]) <= float(a["max_area"]):
        raise bad("min_area", "0 < min_area <= max_area")
    if not float(a["max_area"]) <= 1.0:
        raise bad("max_area", "max_area <= 1")
    if not 0.0 < float(a["min_aspect_ratio"]):
        raise bad("min_aspect_ratio", "0 < min_aspect_ratio")
    if not float(a["min_aspect_ratio"]) <= float(a["max_aspect_ratio"]):
        raise bad("max_aspect_ratio", "min_aspect_ratio <= max_aspect_ratio")
    for field in ("min_object_covered", "overlap_thresh", "random_coef"):
        if not 0.0 <= float(a[field]) <= 1.0:
            raise bad(field, "0 <= %s <= 1" % field)


def _geometric_args(kind, val, args):
    """Builder rules of builders/preprocessor_builder.py:126-228 on a geometric option's filled-in arguments."""
    from . import config
    if kind in ("random_crop_image", "random_crop_pad_image"):
        _check_crop(kind, args)
    if kind in ("random_pad_image", "random_crop_pad_image"):
        color = [float(c) for c in args["pad_color"]]
        if color and len(color) != 3:
            raise ValueError("%s: pad_color should have 3 elements (RGB) if set" % kind)
        args["pad_color"] = color or None
    if kind == "random_pad_image":
        for lim in ("min", "max"):
            hf, wf = lim + "_image_height", lim + "_image_width"
            if (hf in val) != (wf in val):
                raise ValueError("random_pad_image: %s and %s should be either both set or both unset" % (hf, wf))
            args[lim + "_image_size"] = (int(args[hf]), int(args[wf])) if hf in val else None
    elif kind == "random_crop_pad_image":
        for f, d in (("min_padded_size_ratio", (0.0, 0.0)), ("max_padded_size_ratio", (2.0, 2.0))):
            r = [float(v) for v in args[f]]
            if r and len(r) != 2:
                raise ValueError("random_crop_pad_image: %s should have 2 elements if set" % f)
            args[f] = tuple(r) if r else d
    elif kind == "ssd_random_crop":
        defaults = config.DEFAULTS["SSDRandomCropOperation"]
        cases = []
        for i, op in enumerate(args["operations"]):
            unknown = set(op) - set(defaults)
            if unknown:
                raise ValueError("ssd_random_crop: operations[%d] has no field(s) %s" % (i, sorted(unknown)))
            case = {f: op[f] if f in op else d for f, d in defaults.items()}
            _check_crop("ssd_random_crop: operations[%d]" % i, case)
            cases.append(case)
        args["operations"] = cases or [dict(c) for c in _SSD_DEFAULT_CASES]
    return args


def _entries(options):
    for opt in options:
        if hasattr(opt, "keys"):
            for kind in opt.keys():
                yield kind, opt[kind]
        else:
            yield opt, None


def parse_options(options, warn=True, geometric=False):
    """data_augmentation_options (parsed config messages, {kind: {field: value}} dicts or bare option names) ->
    [Step], in config order. Refuses what this path does not run; logs once when an option that clips to [0, 1]
    runs on pixels that no earlier normalize_image mapped to [0, 1] (the reference's own trap: pixels are 0..255
    there, trainer.py:70-73, so such an option alone saturates almost every pixel). geometric=True also accepts the
    GEOMETRIC_KIND options (random crop / pad), which need the multi-task labels made from the boxes."""
    from . import config
    global _warned_range
    steps, unit = [], False
    for kind, val in _entries(options or ()):
        if kind not in OPTION_KIND and not (geometric and kind in GEOMETRIC_KIND):
            raise refusal(kind)
        defaults = config.DEFAULTS[OPTION_KIND.get(kind) or GEOMETRIC_KIND[kind]]
        val = val or {}
        args = {f: (list(val[f]) if isinstance(d, list) else val[f]) if f in val else (list(d) if isinstance(d, list) else d)
                for f, d in defaults.items()}
        unknown = set(val) - set(defaults)
        if unknown:
            raise ValueError("%s has no field(s) %s" % (kind, sorted(unknown)))
        if kind in GEOMETRIC_KIND:
            args = _geometric_args(kind, val, args)
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
        elif k in ("random_crop_image", "ssd_random_crop"):
            codes.append(OP_CROP)
        elif k == "random_pad_image":
            codes.append(OP_PAD)
        elif k == "random_crop_pad_image":
            codes += [OP_CROP, OP_PAD]
    return codes


def num_params(codes):
    return sum(OP_PARAMS[c] for c in codes)


def _uniform(u, lo, hi):
    """tf.random_uniform([], lo, hi) from one draw u in [0, 1): lo + (hi - lo) * u in double, rounded once."""
    return np.float32(float(lo) + (float(hi) - float(lo)) * float(u))


def _seed(u):
    return int(float(u) * 4294967296.0) & 0xFFFFFFFF


def _random_integer(u, lo, hi):
    """core/preprocessor.py:_random_integer = tf.random_uniform([], lo, hi, int32), an integer in [lo, hi), from one
    draw u in [0, 1): lo + floor(u * (hi - lo))."""
    return int(lo) + min(int(float(u) * (int(hi) - int(lo))), int(hi) - int(lo) - 1)


def _plan_crop(a, u_keep, u_seed, H, W, boxes):
    """random_crop_image on an H x W frame -> ((y0, x0, h, w), label action or None). The original is kept when
    u <= random_coef (:841-852), otherwise the window comes from the sampler and the boxes are pruned, moved to its
    frame and clipped (:710-729) even when the sampler fell back to the whole image."""
    if float(u_keep) <= float(a["random_coef"]):
        return (0, 0, H, W), None
    y, x, h, w = sample_crop_window(_seed(u_seed), H, W, boxes, a["min_object_covered"],
                                    (a["min_aspect_ratio"], a["max_aspect_ratio"]), (a["min_area"], a["max_area"]))
    return (y, x, h, w), ("crop", crop_window_box(y, x, h, w, H, W), float(a["overlap_thresh"]))


def _plan_pad(us, H, W, min_size, max_size, color):
    """random_pad_image :895-956 on an H x W frame -> ([offset y, offset x, target h, target w, mode, r, g, b], label
    action). Four draws, used or not: target height, target width, offset y, offset x."""
    max_h, max_w = (2 * H, 2 * W) if max_size is None else max_size
    max_h, max_w = max(int(max_h), H), max(int(max_w), W)
    min_h, min_w = (H, W) if min_size is None else min_size
    min_h, min_w = max(int(min_h), H), max(int(min_w), W)
    th = _random_integer(us[0], min_h, max_h) if max_h > min_h else max_h
    tw = _random_integer(us[1], min_w, max_w) if max_w > min_w else max_w
    oy = _random_integer(us[2], 0, th - H) if th > H else 0
    ox = _random_integer(us[3], 0, tw - W) if tw > W else 0
    window = np.array([-oy, -ox, th - oy, tw - ox], np.float32) / np.array([H, W, H, W], np.float32)
    mode, rgb = (PAD_MEAN, [0.0, 0.0, 0.0]) if color is None else (PAD_GIVEN, [np.float32(c) for c in color])
    return [float(oy), float(ox), float(th), float(tw), mode] + rgb, ("pad", window)


def plan(steps, draws, H, W, boxes, frame=False):
    """-> (float32 [num_params(program(steps))] parameters of one H x W image, label actions) and, with frame=True, the
    (height, width) of the frame after the last option. The draws are the consumer's uniform draws of the example,
    draw_count(steps) of them, in option order. `boxes`: the image's [N, 4] groundtruth boxes, followed through the
    options (the flip's "only if the image has boxes" refers to the boxes at that stage, a second crop samples against
    what the first left); their number is enough when no option moves the frame. Label actions, in config order:
    ("flip", flag), ("jitter", seed, ratio), ("crop", normalised window, overlap_thresh), ("pad", normalised window)."""
    draws = [float(u) for u in draws]
    if len(draws) != draw_count(steps):
        raise ValueError("%d draws for options that take %d" % (len(draws), draw_count(steps)))
    if np.ndim(boxes) == 0:
        if any(s.kind in GEOMETRIC_KIND for s in steps):
            raise ValueError("a geometric option needs the boxes themselves, not their number")
        num_boxes, boxes = int(boxes), None
    else:
        boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        num_boxes = boxes.shape[0]
    it = iter(draws)
    p, actions = [], []
    for s in steps:
        k, a = s.kind, s.args
        done = len(actions)
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
        elif k in GEOMETRIC_KIND:
            if k != "random_pad_image":
                if k == "ssd_random_crop":         # one draw selects the case (:1639-1643)
                    cases = a["operations"]
                    a = cases[min(int(next(it) * len(cases)), len(cases) - 1)]
                crop, act = _plan_crop(a, next(it), next(it), H, W, boxes)
                p += [float(v) for v in crop]
                if act is not None:
                    actions.append(act)
                H0, W0, (H, W) = H, W, crop[2:]
            if k == "random_pad_image":
                sizes = a["min_image_size"], a["max_image_size"]
            elif k == "random_crop_pad_image":     # ratios of the size BEFORE the crop (:1037-1042), truncated
                sizes = [(int(np.float32(H0) * np.float32(r[0])), int(np.float32(W0) * np.float32(r[1])))
                         for r in (a["min_padded_size_ratio"], a["max_padded_size_ratio"])]
            if k in ("random_pad_image", "random_crop_pad_image"):
                pad, act = _plan_pad([next(it) for _ in range(4)], H, W, sizes[0], sizes[1], a["pad_color"])
                p += pad
                actions.append(act)
                H, W = int(pad[2]), int(pad[3])
        if boxes is not None:                      # the boxes the next option sees
            for act in actions[done:]:
                boxes = _act_on_boxes(boxes, act)[0]
            num_boxes = boxes.shape[0]
    out = np.array(p, np.float32), actions
    return out + ((int(H), int(W)),) if frame else out


def _act_on_boxes(boxes, act):
    """One label action on [N, 4] boxes -> (boxes, indices of the kept rows or None when every row stays)."""
    if act[0] == "flip":
        return (flip_boxes(boxes) if act[1] else boxes), None
    if act[0] == "jitter":
        return jitter_boxes(boxes, act[1], act[2]), None
    if act[0] == "crop":
        return crop_boxes(boxes, act[1], act[2])
    if act[0] == "pad":
        return change_coordinate_frame(boxes, act[1]), None
    raise ValueError("bad label action %r" % (act,))


# ------------------------------------------------------------------------------ geometric labels (box_list_ops.py)
def box_area(boxes):
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def prune_completely_outside_window(boxes, window):
    """box_list_ops.py:172-200: drops the boxes with no interior point in the window (the comparisons include
    equality) -> (boxes, kept indices)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    w = np.asarray(window, np.float32)
    out = (b[:, 0] >= w[2]) | (b[:, 1] >= w[3]) | (b[:, 2] <= w[0]) | (b[:, 3] <= w[1])
    idx = np.nonzero(~out)[0]
    return b[idx], idx


def ioa(boxes1, boxes2):
    """box_list_ops.py:296-314: [N, M] intersection of box1 n and box2 m over the area of box2 m."""
    a = np.asarray(boxes1, np.float32).reshape(-1, 4)
    b = np.asarray(boxes2, np.float32).reshape(-1, 4)
    ih = np.maximum(_F(0), np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]))
    iw = np.maximum(_F(0), np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]))
    with np.errstate(all="ignore"):
        return ((ih * iw) / box_area(b)[None, :]).astype(np.float32)


def prune_non_overlapping_boxes(boxes1, boxes2, min_overlap=0.0):
    """box_list_ops.py:317-342: keeps the boxes of boxes1 whose best ioa with a box of boxes2 (over their OWN area) is
    >= min_overlap -> (boxes, kept indices). A box of zero area has ioa 0/0 and is dropped, as in the reference."""
    b = np.asarray(boxes1, np.float32).reshape(-1, 4)
    r = ioa(boxes2, b)
    best = r.max(axis=0) if r.shape[0] else np.full(b.shape[0], -np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(best >= _F(min_overlap))[0]
    return b[idx], idx


def change_coordinate_frame(boxes, window):
    """box_list_ops.py:363-390: boxes relative to the window [ymin, xmin, ymax, xmax]: subtract its corner, then
    multiply by float32(1 / height) and float32(1 / width)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    w = np.asarray(window, np.float32)
    with np.errstate(all="ignore"):
        sy, sx = _F(1.0) / (w[2] - w[0]), _F(1.0) / (w[3] - w[1])
    return ((b - np.stack([w[0], w[1], w[0], w[1]])) * np.stack([sy, sx, sy, sx])).astype(np.float32)


def crop_boxes(boxes, window, overlap_thresh):
    """The label side of _strict_random_crop_image (core/preprocessor.py:710-729): prune the boxes completely outside
    the crop window, prune those the crop covers less than overlap_thresh of, change the frame, clip to [0, 1] ->
    (boxes, indices of the kept rows of the input)."""
    b, i1 = prune_completely_outside_window(boxes, window)
    b, i2 = prune_non_overlapping_boxes(b, np.asarray(window, np.float32).reshape(1, 4), overlap_thresh)
    b = change_coordinate_frame(b, window)
    return np.minimum(np.maximum(b, _F(0)), _F(1)), i1[i2]


def crop_window_box(y, x, h, w, H, W):
    """The normalised box of the pixel window: float32 [y/H, x/W, (y+h)/H, (x+w)/W]."""
    return np.array([y, x, y + h, x + w], np.float32) / np.array([H, W, H, W], np.float32)


def _lrint(v):
    return int(np.rint(v))                                  # round half to even, like C lrintf in the default mode


def crop_attempt(u, H, W, aspect_ratio_range, area_range):
    """One attempt of the crop-window sampler from its four uniforms (float32) -> (y, x, h, w) or None when the
    attempt is rejected before the coverage test. All arithmetic in float32, after TF 1.7's
    sample_distorted_bounding_box_op.cc GenerateRandomCrop."""
    f = np.float32
    aspect = f(aspect_ratio_range[0]) + f(u[0]) * (f(aspect_ratio_range[1]) - f(aspect_ratio_range[0]))
    min_area = f(area_range[0]) * f(W) * f(H)
    max_area = f(area_range[1]) * f(W) * f(H)
    h = _lrint(np.sqrt(min_area / aspect))
    max_h = _lrint(np.sqrt(max_area / aspect))
    if _lrint(f(max_h) * aspect) > W:
        max_h = int(((f(W) + f(0.5)) - f(1e-7)) / aspect)
    max_h = min(max_h, H)
    h = min(h, max_h)
    if h < max_h:
        h += int(np.floor(f(u[1]) * f(max_h - h + 1)))
    w = _lrint(f(h) * aspect)
    if f(w * h) < min_area:
        h += 1
        w = _lrint(f(h) * aspect)
    if f(w * h) > max_area:
        h -= 1
        w = _lrint(f(h) * aspect)
    area = f(w * h)
    if area < min_area or area > max_area or w > W or h > H or w <= 0 or h <= 0:
        return None
    y = int(np.floor(f(u[2]) * f(H - h))) if h < H else 0
    x = int(np.floor(f(u[3]) * f(W - w))) if w < W else 0
    return y, x, h, w


def crop_covers(window, rects, min_object_covered):
    """Whether the crop (y, x, h, w) meets some pixel rectangle (y0, x0, y1, x1) of positive area in positive area and
    covers at least min_object_covered of it (float32 quotient)."""
    y, x, h, w = window
    for y0, x0, y1, x1 in rects:
        ra = (y1 - y0) * (x1 - x0)
        ih, iw = min(y + h, y1) - max(y, y0), min(x + w, x1) - max(x, x0)
        if ra > 0 and ih > 0 and iw > 0 and _F(ih * iw) / _F(ra) >= _F(min_object_covered):
            return True
    return False


def sample_crop_window(seed, H, W, boxes, min_object_covered, aspect_ratio_range, area_range, max_attempts=100,
                       return_attempt=False):
    """The crop window (y, x, h, w) of an H x W image for tf.image.sample_distorted_bounding_box(image_shape, boxes
    clipped to [0, 1], min_object_covered, aspect_ratio_range, area_range, max_attempts=100,
    use_image_if_no_bounding_boxes=True), as _strict_random_crop_image :691-698 calls it. The boxes become pixel
    rectangles with truncated corners int(coordinate * size); an image without boxes has the whole image as its one
    rectangle. Attempt a takes the uniforms hash_uniform(seed, CROP_STREAM, 4 a + j), j = 0..3 (crop_attempt), and is
    accepted when crop_covers holds; after max_attempts rejections the crop is the whole image. This definition is
    the contract: TensorFlow's kernel is not in the reference, its parity is unpinned. return_attempt=True appends the
    index of the accepted attempt (max_attempts for the fallback)."""
    b = np.minimum(np.maximum(np.asarray(boxes, np.float32).reshape(-1, 4), _F(0)), _F(1))
    size = np.array([H, W, H, W], np.float32)
    rects = [tuple(int(v) for v in r) for r in (b * size)] or [(0, 0, H, W)]
    u = hash_uniform(seed, CROP_STREAM, np.arange(4 * max_attempts, dtype=np.uint64)).reshape(-1, 4)
    for a in range(max_attempts):
        win = crop_attempt(u[a], H, W, aspect_ratio_range, area_range)
        if win is not None and crop_covers(win, rects, min_object_covered):
            return win + (a,) if return_attempt else win
    return (0, 0, H, W) + ((max_attempts,) if return_attempt else ())


def stage_frames(codes, params, H, W):
    """The (height, width) of the frame before each op of an H x W image's program, then the final frame."""
    frames, k = [], 0
    for code in codes:
        frames.append((int(H), int(W)))
        if code in GEOMETRIC_OPS:
            H, W = int(params[k + 2]), int(params[k + 3])
        k += OP_PARAMS[code]
    return frames + [(int(H), int(W))]


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
    """Per-channel mean of a float32 [H,W,3] frame for adjust_contrast and the mean-coloured pad: float64 sums, x
    ascending within a row, then the row sums ascending, divided by H*W and rounded once to float32 (the device pre-pass
    of a mean slot, k_aug_rowsum / k_aug_mean, adds in the same order). np.cumsum adds sequentially; np.sum would add
    pairwise."""
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
    pixel scale, the contrast mean, the mean colour of a pad) use the image as it is at that stage: OP_CROP is the
    slice, OP_PAD the array filled with the pad colour around the image."""
    x = np.asarray(image)
    params = np.asarray(params, np.float32)
    k = 0
    for code in codes:
        p = params[k:k + OP_PARAMS[code]]
        k += OP_PARAMS[code]
        H, W = x.shape[:2]
        if code == OP_FLIP:
            if p[0] != 0:
                x = x[:, ::-1].copy()
            continue
        if code == OP_CROP:
            y0, x0, h, w = (int(v) for v in p)
            if not (0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= H and x0 + w <= W):
                raise ValueError("crop %s leaves its %d x %d frame" % ((y0, x0, h, w), H, W))
            x = x[y0:y0 + h, x0:x0 + w].copy()
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
        elif code == OP_PAD:
            oy, ox, th, tw = (int(v) for v in p[:4])
            if not (0 <= oy and 0 <= ox and oy + H <= th and ox + W <= tw):
                raise ValueError("pad %s does not hold its %d x %d frame" % ((oy, ox, th, tw), H, W))
            color = contrast_mean(x) if p[4] != 0 else p[5:8]
            padded = np.empty((th, tw, 3), np.float32)
            padded[:] = np.asarray(color, np.float32)
            padded[oy:oy + H, ox:ox + W] = x
            x = padded
        else:
            raise ValueError("bad augmentation op code %r" % code)
    if k != params.size:
        raise ValueError("%d parameters for a program that takes %d" % (params.size, k))
    return x


def apply_labels(ex, actions):
    """The label side of plan()'s actions on one example dict (flips of boxes, window boxes and edge mask; box
    jitter of groundtruth_boxes only, get_default_func_arg_map; a crop prunes and moves groundtruth_boxes and gathers
    groundtruth_classes / groundtruth_difficult with the kept rows; a pad moves groundtruth_boxes)."""
    ex = dict(ex)
    for act in actions:
        if act[0] in ("crop", "pad"):
            ex["groundtruth_boxes"], keep = _act_on_boxes(ex["groundtruth_boxes"], act)
            for f in ("groundtruth_classes", "groundtruth_difficult"):
                if keep is not None and ex.get(f) is not None:
                    ex[f] = np.asarray(ex[f])[keep]
        elif act[0] == "flip":
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


def drop_aux_fields(ex):
    """An example without the auxiliary labels frozen into its record (AUX_FIELDS): after a geometric option they
    would be in the old frame, so nothing stale can be consumed."""
    return {k: v for k, v in ex.items() if k not in AUX_FIELDS}


def preprocess(example, data_augmentation_options, rng=None, geometric=False):
    """core/preprocessor.py:1905-2048 `preprocess(tensor_dict, preprocess_options)` for the options that only touch
    pixels, random_jitter_boxes and random_horizontal_flip, in config order. `example`: one image's dict with the
    fields of mtl_ssl_amd.synthetic.make_batch (unbatched): image, groundtruth_boxes, window_boxes,
    groundtruth_edgemask (class / closeness labels are invariant under these options). Every option takes a fixed
    number of rng.uniform() draws (Step.draws), taken up front in option order. geometric=True also runs the random
    crop / pad options (GEOMETRIC_KIND) and drops the example's frozen auxiliary labels (AUX_FIELDS)."""
    steps = parse_options(data_augmentation_options, geometric=geometric)
    rng = rng if rng is not None else np.random
    draws = [float(rng.uniform()) for _ in range(draw_count(steps))]
    image = np.asarray(example["image"])
    params, actions = plan(steps, draws, image.shape[0], image.shape[1],
                           np.asarray(example["groundtruth_boxes"], np.float32).reshape(-1, 4))
    ex = apply_labels(drop_aux_fields(example) if geometric else example, actions)
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
