"""CPU tests of the photometric augmentations (mtl_ssl_amd/preprocessor.py): config parsing with the proto defaults,
the refusals, the fixed draw counts (and a flip-only config drawing exactly what it drew before), known answers of
every op, the HSV restatement of TF 1.7's adjust_hue / adjust_saturation kernels against Python's colorsys in
float64 (TF cannot run here: these pin the restatement), box jitter, and the asynchronous pipeline's host preparer
against input_reader.batches for a config that lists every supported option with flips in between."""
import colorsys
import io
import logging
import os

import numpy as np
import pytest
import torch

from mtl_ssl_amd import config
from mtl_ssl_amd import input_pipeline as IP
from mtl_ssl_amd import input_reader as R
from mtl_ssl_amd import preprocessor as P

K = 3
ALL_OPTIONS = """
train_config {
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 255 target_minval: 0 target_maxval: 1 } }
  data_augmentation_options { random_horizontal_flip { } }
  data_augmentation_options { random_adjust_brightness { max_delta: 0.1 } }
  data_augmentation_options { random_adjust_contrast { } }
  data_augmentation_options { random_horizontal_flip { } }
  data_augmentation_options { random_adjust_saturation { } }
  data_augmentation_options { random_adjust_hue { } }
  data_augmentation_options { random_distort_color { color_ordering: 1 } }
  data_augmentation_options { random_rgb_to_gray { probability: 0.5 } }
  data_augmentation_options { random_pixel_value_scale { } }
  data_augmentation_options { random_black_patches { max_black_patches: 4 probability: 0.7 } }
  data_augmentation_options { random_horizontal_flip { } }
  data_augmentation_options { random_jitter_boxes { } }
  data_augmentation_options { subtract_channel_mean { means: [0.1, 0.2, 0.3] } }
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 1 target_minval: 0 target_maxval: 255 } }
}
"""


def _opts(text):
    return config.parse_pipeline_config(text).train_config.data_augmentation_options


def _one(kind, body=""):
    return _opts("train_config { data_augmentation_options { %s { %s } } }" % (kind, body))


def test_every_option_parses_with_its_defaults_and_overrides():
    want = {"normalize_image": {"original_minval": 0.0, "original_maxval": 0.0, "target_minval": 0, "target_maxval": 1},
            "subtract_channel_mean": {"means": []}, "random_adjust_brightness": {"max_delta": 0.2},
            "random_adjust_contrast": {"min_delta": 0.8, "max_delta": 1.25},
            "random_adjust_saturation": {"min_delta": 0.8, "max_delta": 1.25}, "random_adjust_hue": {"max_delta": 0.02},
            "random_distort_color": {"color_ordering": 0}, "random_rgb_to_gray": {"probability": 0.1},
            "random_pixel_value_scale": {"minval": 0.9, "maxval": 1.1},
            "random_black_patches": {"max_black_patches": 10, "probability": 0.5, "size_to_image_ratio": 0.1},
            "random_jitter_boxes": {"ratio": 0.05}, "random_horizontal_flip": {}}
    for kind, args in want.items():
        if kind in ("normalize_image", "subtract_channel_mean"):
            continue                                   # no usable defaults: checked with overrides below
        (step,) = P.parse_options(_one(kind), warn=False)
        assert (step.kind, step.args) == (kind, args)
        msg = _one(kind)[0][kind]                      # the parsed message carries the proto defaults too
        for f, v in args.items():
            assert getattr(msg, f) == v, (kind, f)
    steps = P.parse_options(_opts(ALL_OPTIONS), warn=False)
    assert [s.kind for s in steps] == [
        "normalize_image", "random_horizontal_flip", "random_adjust_brightness", "random_adjust_contrast",
        "random_horizontal_flip", "random_adjust_saturation", "random_adjust_hue", "random_distort_color",
        "random_rgb_to_gray", "random_pixel_value_scale", "random_black_patches", "random_horizontal_flip",
        "random_jitter_boxes", "subtract_channel_mean", "normalize_image"]
    assert steps[0].args == {"original_minval": 0, "original_maxval": 255, "target_minval": 0, "target_maxval": 1}
    assert steps[2].args == {"max_delta": 0.1}
    assert steps[7].args == {"color_ordering": 1}
    assert steps[10].args == {"max_black_patches": 4, "probability": 0.7, "size_to_image_ratio": 0.1}
    assert steps[13].args == {"means": [0.1, 0.2, 0.3]}
    # plain dicts (and bare names) work like parsed messages
    (s,) = P.parse_options([{"random_adjust_hue": {"max_delta": 0.3}}], warn=False)
    assert s.args == {"max_delta": 0.3}
    assert P.parse_options(["random_horizontal_flip"], warn=False)[0].kind == "random_horizontal_flip"


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError, match="original_maxval != original_minval"):
        P.parse_options(_one("normalize_image"))
    with pytest.raises(ValueError, match="len\\(means\\)"):
        P.parse_options(_one("subtract_channel_mean", "means: [1, 2]"))
    with pytest.raises(ValueError, match="color_ordering"):
        P.parse_options(_one("random_distort_color", "color_ordering: 2"))
    with pytest.raises(ValueError, match="no field"):
        P.parse_options([{"random_adjust_hue": {"max_dleta": 0.1}}])


@pytest.mark.parametrize("kind,why", [
    ("random_crop_image", "old frame"), ("random_pad_image", "old frame"), ("random_crop_pad_image", "old frame"),
    ("random_crop_to_aspect_ratio", "old frame"), ("ssd_random_crop", "old frame"), ("ssd_random_crop_pad", "old frame"),
    ("ssd_random_crop_fixed_aspect_ratio", "old frame"), ("random_image_scale", "resize_to_range"),
    ("random_resize_method", "resize_to_range"), ("resize_image", "resize_to_range"),
    ("scale_boxes_to_pixel_coordinates", "normalised boxes"), ("random_crop", "no PreprocessingStep option")])
def test_refusals_say_why(kind, why):
    for parse in (lambda: P.parse_options([{kind: {}}]), lambda: IP.option_draw_counts([kind]),
                  lambda: P.preprocess({"image": np.zeros((2, 2, 3), np.float32),
                                        "groundtruth_boxes": np.zeros((0, 4), np.float32)}, [kind])):
        with pytest.raises(ValueError, match="not supported: .*" + why):
            parse()


def test_draw_counts_are_fixed_per_option():
    counts = {"random_horizontal_flip": 1, "normalize_image": 0, "subtract_channel_mean": 0,
              "random_adjust_brightness": 1, "random_adjust_contrast": 1, "random_adjust_saturation": 1,
              "random_adjust_hue": 1, "random_distort_color": 4, "random_rgb_to_gray": 1,
              "random_pixel_value_scale": 1, "random_black_patches": 30, "random_jitter_boxes": 1}
    args = {"normalize_image": {"original_minval": 0, "original_maxval": 255},
            "subtract_channel_mean": {"means": [1, 2, 3]}}
    for kind, n in counts.items():
        assert IP.option_draw_counts([{kind: args.get(kind, {})}]) == [n], kind
    assert IP.option_draw_counts([{"random_black_patches": {"max_black_patches": 4}}]) == [12]
    assert IP.option_draw_counts(_opts(ALL_OPTIONS)) == [0, 1, 1, 1, 1, 1, 1, 4, 1, 1, 12, 1, 1, 0, 0]
    # the draws do not depend on the pixels or the number of boxes
    opts = _opts(ALL_OPTIONS)
    for G in (0, 1, 7):
        for hw in ((5, 9), (40, 30)):
            rng = np.random.RandomState(3)
            P.preprocess({"image": np.full(hw + (3,), 7.0, np.float32), "groundtruth_boxes": np.full((G, 4), 0.5, np.float32)},
                         opts, rng)
            ref = np.random.RandomState(3)
            ref.uniform(size=26)
            assert rng.uniform() == ref.uniform()


def test_flip_only_configs_draw_and_flip_as_before():
    """One rng.uniform() per listed flip, flipped when u > 0.5 and the image has boxes; the image keeps its dtype."""
    img = np.arange(2 * 5 * 3, dtype=np.float32).reshape(2, 5, 3)
    boxes = np.array([[0.1, 0.2, 0.5, 0.6]], np.float32)
    wins = np.array([[0.0, 0.1, 0.4, 0.3]], np.float32)
    em = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    flip2 = _one("random_horizontal_flip") + _one("random_horizontal_flip")
    for seed in range(20):
        rng, ref = np.random.RandomState(seed), np.random.RandomState(seed)
        ex = dict(image=img, groundtruth_boxes=boxes, window_boxes=wins, groundtruth_edgemask=em)
        got = P.preprocess(ex, flip2, rng)
        want = dict(ex)
        for _ in range(2):                      # the flip path as it was: random_horizontal_flip per option
            res = P.random_horizontal_flip(want["image"], want["groundtruth_boxes"], want["window_boxes"],
                                           want["groundtruth_edgemask"], ref)
            want = dict(want, image=res[0], groundtruth_boxes=res[1], window_boxes=res[2], groundtruth_edgemask=res[3])
        assert rng.uniform() == ref.uniform()
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (seed, k)
    u8 = P.preprocess(dict(image=np.zeros((2, 3, 3), np.uint8), groundtruth_boxes=boxes), flip2,
                      np.random.RandomState(0))["image"]
    assert u8.dtype == np.uint8


def _prog(options, draws, H=4, W=5, boxes=1):
    steps = P.parse_options(options, warn=False)
    params, actions = P.plan(steps, draws, H, W, boxes)
    return P.program(steps), params, actions


def test_normalize_channel_mean_and_brightness_arithmetic():
    x = np.random.RandomState(0).randint(0, 256, (4, 5, 3)).astype(np.float32)
    codes, params, _ = _prog(_opts(ALL_OPTIONS)[:1], [])
    f = np.float32((1.0 - 0.0) / (255.0 - 0.0))
    np.testing.assert_array_equal(P.apply_program(x, codes, params), (x - np.float32(0)) * f + np.float32(0))
    codes, params, _ = _prog([{"normalize_image": {"original_minval": -1, "original_maxval": 3, "target_minval": 10,
                                                   "target_maxval": 11}}], [])
    np.testing.assert_array_equal(params, np.float32([-1, 0.25, 10]))
    codes, params, _ = _prog([{"subtract_channel_mean": {"means": [1.5, 2, 300]}}], [])
    np.testing.assert_array_equal(P.apply_program(x, codes, params), x - np.float32([1.5, 2, 300]))
    # brightness: one draw -> delta = -max_delta + 2 max_delta u, then clip to [0, 1]
    codes, params, _ = _prog([{"random_adjust_brightness": {"max_delta": 0.25}}], [0.75])
    assert codes == [P.OP_ADD, P.OP_CLIP] and params[0] == np.float32(0.125)
    y = np.float32([[[0.1, 0.9, -3.0]]])
    np.testing.assert_array_equal(P.apply_program(y, codes, params), np.float32([[[0.1 + 0.125, 1.0, 0.0]]]).astype(
        np.float32).clip(0, 1) * 0 + np.minimum(np.maximum(y + np.float32(0.125), 0), 1))


def test_gray_weights():
    codes, params, _ = _prog([{"random_rgb_to_gray": {"probability": 0.3}}], [0.3])      # u <= p -> gray
    assert params[0] == 1
    x = np.float32([[[1, 0, 0], [0, 1, 0], [0, 0, 1], [10, 20, 30]]])
    g = P.apply_program(x, codes, params)
    np.testing.assert_array_equal(g[0, :, 0], np.float32([0.2989, 0.5870, 0.1140,
                                                          (np.float32(10) * np.float32(0.2989) + np.float32(20) * np.float32(0.5870))
                                                          + np.float32(30) * np.float32(0.1140)]))
    assert (g == g[..., :1]).all()
    codes, params, _ = _prog([{"random_rgb_to_gray": {"probability": 0.3}}], [0.31])
    np.testing.assert_array_equal(P.apply_program(x, codes, params), x)


def test_hue_and_saturation_known_answers():
    red = np.float32([[[1, 0, 0]]])
    codes, params, _ = _prog([{"random_adjust_hue": {"max_delta": 0.5}}], [(1 / 3 + 0.5)])   # delta = 1/3
    assert abs(params[0] - 1 / 3) < 1e-7
    np.testing.assert_array_equal(P.apply_program(red, codes, params), np.float32([[[0, 1, 0]]]))
    x = np.random.RandomState(1).uniform(0, 1, (6, 7, 3)).astype(np.float32)
    codes, params, _ = _prog([{"random_adjust_saturation": {"min_delta": 0, "max_delta": 1}}], [0.0])     # k = 0
    v = x.max(-1, keepdims=True)
    np.testing.assert_array_equal(P.apply_program(x, codes, params), np.repeat(v, 3, -1))


def test_black_patch_placement_on_a_10x7_image():
    opt = [{"random_black_patches": {"max_black_patches": 2, "probability": 0.5, "size_to_image_ratio": 0.3}}]
    # try 1: u = 0.2 <= 0.5 -> patch at y0 = int(0.5 * 0.7 * 10) = 3, x0 = int(0.9 * 0.7 * 7) = 4, box = int(7 * 0.3) = 2
    # try 2: u = 0.6 > 0.5 -> none
    codes, params, _ = _prog(opt, [0.2, 0.5, 0.9, 0.6, 0.0, 0.0], H=10, W=7)
    np.testing.assert_array_equal(params, np.float32([1, 3, 4, 2, 0, 0, 0, 2]))
    x = np.ones((10, 7, 3), np.float32)
    y = P.apply_program(x, codes, params)
    want = np.ones_like(x)
    want[3:5, 4:6] = 0
    np.testing.assert_array_equal(y, want)
    # a flip before the patches mirrors where it lands in the original frame
    codes, params, _ = _prog([{"random_horizontal_flip": {}}] + opt, [0.9, 0.2, 0.5, 0.9, 0.6, 0.0, 0.0], H=10, W=7)
    y = P.apply_program(x, codes, params)
    np.testing.assert_array_equal(y, want)                       # the patch is placed in the flipped image
    z = P.apply_program(np.arange(70 * 3, dtype=np.float32).reshape(10, 7, 3), codes, params)
    assert (z[3:5, 4:6] == 0).all() and (z != 0).sum() == 70 * 3 - 12 - 1


def test_contrast_mean_is_a_sequential_float64_sum():
    x = np.random.RandomState(2).uniform(0, 1, (37, 53, 3)).astype(np.float32)
    m = P.contrast_mean(x)
    flat = np.cumsum(np.cumsum(x.astype(np.float64), axis=1)[:, -1, :], axis=0)[-1] / (37 * 53)
    np.testing.assert_array_equal(m, flat.astype(np.float32))
    assert m.dtype == np.float32
    codes, params, _ = _prog([{"random_adjust_contrast": {"min_delta": 2, "max_delta": 2}}], [0.5])
    y = P.apply_program(x, codes, params)
    np.testing.assert_array_equal(y, np.minimum(np.maximum((x - m) * np.float32(2) + m, 0), 1))


def _colorsys_hue(px, delta):
    h, s, v = colorsys.rgb_to_hsv(*px)
    return colorsys.hsv_to_rgb((h + delta) % 1.0, s, v)


def _colorsys_saturation(px, k):
    h, s, v = colorsys.rgb_to_hsv(*px)
    return colorsys.hsv_to_rgb(h, min(1.0, max(0.0, s * k)), v)


def test_hsv_ops_against_colorsys():
    rng = np.random.RandomState(5)
    x = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    x[:20] = rng.randint(0, 3, (20, 3)) / np.float32(2)            # ties and grays
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    for delta in (0.0, 0.02, -0.2, 1 / 3, -0.5, 0.4999):
        d = np.float32(delta)
        got = np.stack(P.adjust_hue(r, g, b, d), 1)
        want = np.array([_colorsys_hue(px, float(d)) for px in x.astype(np.float64)])
        assert np.abs(got - want).max() <= 1e-5, delta
    for k in (0.0, 0.5, 1.0, 1.37, 4.0):
        got = np.stack(P.adjust_saturation(r, g, b, np.float32(k)), 1)
        want = np.array([_colorsys_saturation(px, float(np.float32(k))) for px in x.astype(np.float64)])
        assert np.abs(got - want).max() <= 1e-5, k


def test_pixel_value_scale_uses_the_counter_hash():
    codes, params, _ = _prog([{"random_pixel_value_scale": {"minval": 0.5, "maxval": 1.5}}], [0.25], H=3, W=4)
    seed = int(params[:1].view(np.uint32)[0])
    assert seed == int(0.25 * 2 ** 32)
    x = np.full((3, 4, 3), 0.5, np.float32)
    y = P.apply_program(x, codes, params)
    u = P.hash_uniform(seed, P.PIXEL_SCALE_STREAM, np.arange(36))
    np.testing.assert_array_equal(y.reshape(-1), np.minimum(np.maximum(np.float32(0.5) * (np.float32(0.5) + np.float32(1.0) * u), 0), 1))
    assert 0.25 < y.min() and y.max() < 0.75 and len(np.unique(y)) > 30
    # the hash is the samplers' / dropout's mix32 (csrc/glue.hip glue_mix32), restated in 32-bit Python integers
    def mix32(seed, stream, i):
        m = 0xFFFFFFFF
        x = (i + 0x9E3779B9 * seed + 0x85EBCA6B * stream) & m
        x ^= x >> 16
        x = (x * 0x7FEB352D) & m
        x ^= x >> 15
        x = (x * 0x846CA68B) & m
        return x ^ (x >> 16)
    for seed, stream in ((0, 0), (seed, P.PIXEL_SCALE_STREAM), (0xFFFFFFFF, P.JITTER_STREAM)):
        assert [int(v) for v in P.mix32(seed, stream, np.arange(50))] == [mix32(seed, stream, i) for i in range(50)]


def test_jitter_stays_in_bounds_and_is_reproducible():
    boxes = np.array([[0.0, 0.0, 1.0, 1.0], [0.2, 0.3, 0.4, 0.9], [0.5, 0.5, 0.5, 0.5]], np.float32)
    a = P.jitter_boxes(boxes, 1234, 0.05)
    np.testing.assert_array_equal(a, P.jitter_boxes(boxes, 1234, 0.05))
    assert not np.array_equal(a, P.jitter_boxes(boxes, 1235, 0.05))
    assert (a >= 0).all() and (a <= 1).all()
    hw = np.stack([boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]] * 2, 1)[:, [0, 1, 2, 3]]
    assert (np.abs(a - boxes) <= 0.05 * hw + 1e-7).all()
    np.testing.assert_array_equal(a[2], boxes[2])                  # a zero-size box does not move
    # the jitter touches groundtruth_boxes only (get_default_func_arg_map); windows and masks keep their frame
    ex = dict(image=np.zeros((4, 4, 3), np.float32), groundtruth_boxes=boxes, window_boxes=boxes.copy(),
              groundtruth_edgemask=np.ones((2, 3, 3), np.float32))
    out = P.preprocess(ex, _one("random_jitter_boxes", "ratio: 0.1"), np.random.RandomState(0))
    assert not np.array_equal(out["groundtruth_boxes"], boxes)
    np.testing.assert_array_equal(out["window_boxes"], boxes)
    np.testing.assert_array_equal(out["image"], ex["image"])


def test_a_clipping_option_without_normalize_warns_once(caplog, monkeypatch):
    monkeypatch.setattr(P, "_warned_range", False)
    with caplog.at_level(logging.WARNING, logger=P.__name__):
        P.parse_options(_one("random_adjust_brightness"))
        P.parse_options(_one("random_adjust_brightness"))
    assert len([r for r in caplog.records if "normalize_image" in r.getMessage()]) == 1
    monkeypatch.setattr(P, "_warned_range", False)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger=P.__name__):
        P.parse_options(_opts(ALL_OPTIONS))
    assert not caplog.records


def _png(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG")
    return b.getvalue()


def _records(path, shapes, seed):
    rng = np.random.RandomState(seed)
    recs = []
    for i, (h, w) in enumerate(shapes):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        G = int(rng.randint(0, 4))
        y0, x0 = rng.uniform(0, 0.5, G).astype(np.float32), rng.uniform(0, 0.5, G).astype(np.float32)
        y1, x1 = (y0 + rng.uniform(0.1, 0.5, G)).astype(np.float32), (x0 + rng.uniform(0.1, 0.5, G)).astype(np.float32)
        em = rng.rand(2, 4, 5).astype(np.float32)
        recs.append(R.serialize_example({
            "image/encoded": _png(img), "image/format": b"png", "image/filename": "im%d.png" % i,
            "image/source_id": str(i), "image/height": np.array([h]), "image/width": np.array([w]),
            "image/object/bbox/ymin": y0, "image/object/bbox/xmin": x0, "image/object/bbox/ymax": y1,
            "image/object/bbox/xmax": x1, "image/object/class/label": rng.randint(1, K + 1, G).astype(np.int64),
            "image/window/bbox/ymin": y0, "image/window/bbox/xmin": x0, "image/window/bbox/ymax": y1,
            "image/window/bbox/xmax": x1, "image/window/labels/text": [b" ".join([b"0.5"] * (K + 1))] * G,
            "image/edgemask/masks": em.reshape(-1), "image/edgemask/height": np.array([4]),
            "image/edgemask/width": np.array([5])}))
    R.write_tfrecord(path, recs)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        assert torch.equal(g["images"], w["images"])
        for k in w:
            if k != "images":
                assert all((x == y) if isinstance(y, str) else np.array_equal(x, y) for x, y in zip(g[k], w[k])), k


def test_pipeline_with_every_option_equals_the_host_generator(tmp_path):
    p = str(tmp_path / "a.record")
    _records(p, [(12, 16), (16, 12), (20, 30), (9, 13), (16, 12), (12, 16), (25, 25), (7, 11), (20, 30)], 7)
    opts = _opts(ALL_OPTIONS)
    rs = lambda h, w: (max(8, h // 2 * 2), max(8, w // 2 * 2 + 1))
    for kw in (dict(), dict(resized_shape=rs, shuffle_buffer=3, max_pending=3)):
        want = list(R.batches([p], K, 2, opts, rng=np.random.RandomState(4), **kw))
        with IP.InputPipeline([p], K, 2, opts, rng=np.random.RandomState(4), num_workers=3, **kw) as pipe:
            got = list(pipe)
        _same(got, want)
    # the augmented images differ from the plain ones
    plain = list(R.batches([p], K, 2, rng=np.random.RandomState(4)))
    assert not torch.equal(plain[0]["images"], want[0]["images"]) or not torch.equal(plain[1]["images"], want[1]["images"])
