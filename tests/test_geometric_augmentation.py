"""Random crop / pad augmentation on the host (mtl_ssl_amd.preprocessor with geometric=True): the label functions
against the known answers of the reference's own unit tests (tests/golden/geometric_vectors.json, at their
assertAllClose tolerance), the crop-window sampler's contract as properties over 2 000 seeds, the pad's ranges and box
frame, OP_CROP / OP_PAD in apply_program against hand-composed numpy (an option listed before a crop sees the uncropped
frame), fixed draw counts, the opt-in gating with the train-time rule, and the two record feeds against each other."""
import io
import json
import os

import numpy as np
import pytest

from mtl_ssl_amd import config
from mtl_ssl_amd import input_pipeline as IP
from mtl_ssl_amd import input_reader as R
from mtl_ssl_amd import preprocessor as P
from mtl_ssl_amd import train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "geometric_vectors.json")) as _f:
    GOLD = json.load(_f)
TOL = dict(rtol=GOLD["tolerance"]["rtol"], atol=GOLD["tolerance"]["atol"])
F = np.float32
GEO = ("random_crop_image", "random_pad_image", "random_crop_pad_image", "ssd_random_crop")


def _opts(text):
    return config.parse_pipeline_config("train_config { %s }" % " ".join(
        "data_augmentation_options { %s }" % t for t in text)).train_config.data_augmentation_options


# ------------------------------------------------------------------------------ known answers of the reference
@pytest.mark.parametrize("case", GOLD["crop"]["cases"], ids=lambda c: c["name"])
def test_crop_labels_match_the_reference_unit_tests(case):
    g = GOLD["crop"]
    (H, W), (y, x), (h, w) = g["image_size"], g["begin"], g["size"]
    np.testing.assert_allclose(P.crop_window_box(y, x, h, w, H, W), g["box"], **TOL)
    boxes, keep = P.crop_boxes(F(case["boxes"]), F(g["box"]), g["overlap_thresh"])
    np.testing.assert_allclose(boxes, case["expected_boxes"], **TOL)
    assert list(np.asarray(case["labels"])[keep]) == case["expected_labels"]
    # through the label action, with the window given and not sampled
    onehot = np.eye(12, dtype=F)[case["labels"]]
    ex = P.apply_labels(dict(groundtruth_boxes=F(case["boxes"]), groundtruth_classes=onehot,
                             groundtruth_difficult=np.arange(len(onehot)) % 2 == 0),
                        [("crop", F(g["box"]), g["overlap_thresh"])])
    np.testing.assert_allclose(ex["groundtruth_boxes"], case["expected_boxes"], **TOL)
    assert list(ex["groundtruth_classes"].argmax(1)) == case["expected_labels"]
    np.testing.assert_array_equal(ex["groundtruth_difficult"], (np.arange(len(onehot)) % 2 == 0)[keep])


def test_box_list_ops_vectors():
    g = GOLD["prune_completely_outside_window"]
    boxes, idx = P.prune_completely_outside_window(g["boxes"], g["window"])
    np.testing.assert_allclose(boxes, g["expected_boxes"], **TOL)
    assert list(idx) == g["expected_indices"]
    g = GOLD["ioa"]
    np.testing.assert_allclose(P.ioa(g["boxes1"], g["boxes2"]), g["expected_1_2"], **TOL)
    np.testing.assert_allclose(P.ioa(g["boxes2"], g["boxes1"]), g["expected_2_1"], **TOL)
    g = GOLD["prune_non_overlapping_boxes"]
    out, idx = P.prune_non_overlapping_boxes(g["boxes1"], g["boxes2"], g["min_overlap"])
    np.testing.assert_allclose(out, g["boxes1"], **TOL)
    assert list(idx) == g["expected_indices_1"]
    out, idx = P.prune_non_overlapping_boxes(g["boxes2"], g["boxes1"], g["min_overlap"])
    assert out.shape == (0, 4) and list(idx) == g["expected_indices_2"]
    g = GOLD["change_coordinate_frame"]
    np.testing.assert_allclose(P.change_coordinate_frame(g["boxes"], g["window"]), g["expected_boxes"], **TOL)


# ------------------------------------------------------------------------------ the sampler's contract
H0, W0 = 61, 83
BOXES = F([[0.1, 0.1, 0.6, 0.5], [0.3, 0.4, 0.9, 0.9]])
SAMPLER_CASES = [(0.5, (0.75, 1.33), (0.1, 1.0)), (1.0, (0.5, 2.0), (0.3, 0.9)), (0.0, (0.75, 1.33), (0.05, 0.5))]


def _rects(boxes, H, W):
    b = np.clip(F(boxes).reshape(-1, 4), 0, 1) * F([H, W, H, W])
    return [tuple(int(v) for v in r) for r in b] or [(0, 0, H, W)]


# Without boxes the one rectangle is the whole image, so the coverage condition reads crop area / image area >=
# min_object_covered: it holds for every crop of the area range when min_object_covered is below the range's lower end
# (and can never hold when it is above the upper end), so these cases must never fall back.
NO_BOX_CASES = [(0.0, (0.75, 1.33), (0.05, 0.5)), (0.05, (0.5, 2.0), (0.1, 1.0))]
NONE = np.zeros((0, 4), F)


@pytest.mark.parametrize("boxes,covered,ar,area", [(BOXES,) + c for c in SAMPLER_CASES] + [(NONE,) + c for c in NO_BOX_CASES])
def test_sampler_properties(boxes, covered, ar, area):
    fallbacks = 0
    for seed in range(2000):
        y, x, h, w, attempt = P.sample_crop_window(seed, H0, W0, boxes, covered, ar, area, return_attempt=True)
        assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= H0 and x + w <= W0, (seed, y, x, h, w)
        if attempt == 100:
            fallbacks += 1
            assert (y, x, h, w) == (0, 0, H0, W0)
            continue
        assert F(area[0]) * F(W0) * F(H0) <= F(w * h) <= F(area[1]) * F(W0) * F(H0), (seed, h, w)
        u0 = P.hash_uniform(seed, P.CROP_STREAM, np.uint64(4 * attempt))
        aspect = F(ar[0]) + u0 * (F(ar[1]) - F(ar[0]))
        assert w == int(np.rint(F(h) * aspect)), (seed, h, w, aspect)
        assert P.crop_covers((y, x, h, w), _rects(boxes, H0, W0), covered), seed
    # measured on the host sampler before the cap was written: 0 of 2 000 for every case with boxes
    assert fallbacks < 0.05 * 2000, fallbacks
    if len(boxes) == 0:
        assert fallbacks == 0


def test_sampler_falls_back_to_the_whole_image_and_is_deterministic():
    tiny = F([[0.0, 0.0, 1.0, 1.0]])              # the crop must cover ALL of a box that fills the image: area <= 0.5 never does
    assert P.sample_crop_window(7, H0, W0, tiny, 1.0, (0.75, 1.33), (0.1, 0.5)) == (0, 0, H0, W0)
    a = [P.sample_crop_window(s, H0, W0, BOXES, 0.5, (0.75, 1.33), (0.1, 1.0)) for s in range(20)]
    assert a == [P.sample_crop_window(s, H0, W0, BOXES, 0.5, (0.75, 1.33), (0.1, 1.0)) for s in range(20)]
    assert len(set(a)) > 10


# ------------------------------------------------------------------------------ pad
@pytest.mark.parametrize("fields,color", [("", None), ("min_image_height: 70 min_image_width: 40 max_image_height: 90 "
                                                        "max_image_width: 200 pad_color: [0.25, 3, 200]", [0.25, 3, 200]),
                                           ("max_image_height: 10 max_image_width: 10", None)])
def test_pad_ranges_boxes_and_colour(fields, color):
    steps = P.parse_options(_opts(["random_pad_image { %s }" % fields]), geometric=True)
    a = steps[0].args
    lo = (max(a["min_image_size"][0], H0), max(a["min_image_size"][1], W0)) if a["min_image_size"] else (H0, W0)
    hi = (max(a["max_image_size"][0], H0), max(a["max_image_size"][1], W0)) if a["max_image_size"] else (2 * H0, 2 * W0)
    rng = np.random.RandomState(1)
    img = rng.randint(0, 256, (H0, W0, 3)).astype(F)
    for _ in range(200):
        params, actions, frame = P.plan(steps, rng.uniform(size=4), H0, W0, BOXES, frame=True)
        oy, ox, th, tw = (int(v) for v in params[:4])
        assert frame == (th, tw) and lo[0] <= th <= hi[0] and lo[1] <= tw <= hi[1]
        assert th < hi[0] or hi[0] == lo[0]
        assert 0 <= oy <= th - H0 and 0 <= ox <= tw - W0
        (kind, window), = actions
        assert kind == "pad"
        np.testing.assert_array_equal(window, F([-oy, -ox, th - oy, tw - ox]) / F([H0, W0, H0, W0]))
        got = P.apply_labels(dict(groundtruth_boxes=BOXES, groundtruth_classes=np.eye(2, dtype=F)), actions)
        np.testing.assert_array_equal(got["groundtruth_boxes"], P.change_coordinate_frame(BOXES, window))
        # the same boxes in pixels of the padded frame, to the rounding of two float32 steps
        np.testing.assert_allclose(got["groundtruth_boxes"] * [th, tw, th, tw],
                                   BOXES * [H0, W0, H0, W0] + [oy, ox, oy, ox], rtol=1e-5, atol=1e-4)
        assert len(got["groundtruth_classes"]) == 2
        out = P.apply_program(img, P.program(steps), params)
        want = np.empty((th, tw, 3), F)
        want[:] = F(color) if color else P.contrast_mean(img)
        want[oy:oy + H0, ox:ox + W0] = img
        np.testing.assert_array_equal(out, want)
        assert params[4] == (P.PAD_GIVEN if color else P.PAD_MEAN)
    if fields.startswith("max_image_height: 10"):           # limits below the image: the image size, no padding
        assert frame == (H0, W0) and (oy, ox) == (0, 0)


def test_pad_builder_rules():
    with pytest.raises(ValueError, match="min_image_height and min_image_width .*both set or both unset"):
        P.parse_options(_opts(["random_pad_image { min_image_height: 5 }"]), geometric=True)
    with pytest.raises(ValueError, match="max_image_height and max_image_width .*both set or both unset"):
        P.parse_options(_opts(["random_pad_image { max_image_width: 5 }"]), geometric=True)
    with pytest.raises(ValueError, match="pad_color should have 3"):
        P.parse_options(_opts(["random_pad_image { pad_color: [1, 2] }"]), geometric=True)
    with pytest.raises(ValueError, match="min_padded_size_ratio should have 2"):
        P.parse_options(_opts(["random_crop_pad_image { min_padded_size_ratio: [1] }"]), geometric=True)


def test_crop_pad_sizes_are_ratios_of_the_uncropped_image():
    steps = P.parse_options(_opts(["random_crop_pad_image { min_padded_size_ratio: [1.5, 1.5] "
                                   "max_padded_size_ratio: [1.5, 1.5] max_area: 0.5 }"]), geometric=True)
    rng = np.random.RandomState(2)
    for _ in range(50):
        params, actions, frame = P.plan(steps, rng.uniform(size=6), H0, W0, BOXES, frame=True)
        assert frame == (int(F(H0) * F(1.5)), int(F(W0) * F(1.5)))
        assert params[2] * params[3] <= 0.5 * H0 * W0 and params[8] == P.PAD_MEAN
        assert [a[0] for a in actions] == ["crop", "pad"]


# ------------------------------------------------------------------------------ apply_program
def test_crop_and_pad_in_apply_program_and_order_matters():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (H0, W0, 3)).astype(F)
    crop = F([5, 7, 30, 41])
    np.testing.assert_array_equal(P.apply_program(img, [P.OP_CROP], crop), img[5:35, 7:48])
    np.testing.assert_array_equal(P.apply_program(img, [P.OP_CROP], F([0, 0, H0, W0])), img)
    with pytest.raises(ValueError, match="leaves its"):
        P.apply_program(img, [P.OP_CROP], F([40, 0, 30, 41]))
    scale = np.concatenate([np.uint32([1234]).view(F), F([0.9, 0.2])])

    def u(h, w):
        return P.hash_uniform(1234, P.PIXEL_SCALE_STREAM, np.arange(h * w * 3, dtype=np.uint64)).reshape(h, w, 3)
    before = P.apply_program(img, [P.OP_PIXEL_SCALE, P.OP_CROP], np.concatenate([scale, crop]))
    after = P.apply_program(img, [P.OP_CROP, P.OP_PIXEL_SCALE], np.concatenate([crop, scale]))
    np.testing.assert_array_equal(before, (img * (F(0.9) + F(0.2) * u(H0, W0)))[5:35, 7:48])
    np.testing.assert_array_equal(after, img[5:35, 7:48] * (F(0.9) + F(0.2) * u(30, 41)))
    assert not np.array_equal(before, after)
    # contrast after a mean-coloured pad takes its mean over the padded frame
    pad = F([3, 4, 40, 50, P.PAD_MEAN, 0, 0, 0])
    got = P.apply_program(img, [P.OP_CROP, P.OP_PAD, P.OP_CONTRAST], np.concatenate([crop, pad, F([1.5])]))
    x = np.empty((40, 50, 3), F)
    x[:] = P.contrast_mean(img[5:35, 7:48])
    x[3:33, 4:45] = img[5:35, 7:48]
    m = P.contrast_mean(x)
    np.testing.assert_array_equal(got, (x - m) * F(1.5) + m)
    assert P.stage_frames([P.OP_CROP, P.OP_PAD, P.OP_CONTRAST], np.concatenate([crop, pad, F([1.5])]), H0, W0) == [
        (H0, W0), (30, 41), (40, 50), (40, 50)]


def test_plan_follows_the_boxes_through_the_options():
    # a crop that prunes every box (overlap_thresh 1 on boxes the crop cannot hold), then a flip: never flipped
    steps = P.parse_options(_opts(["random_crop_image { min_object_covered: 0 max_area: 0.11 overlap_thresh: 1 }",
                                   "random_horizontal_flip { }"]), geometric=True)
    big = F([[0.0, 0.0, 1.0, 1.0]])
    for seed in range(20):
        params, actions = P.plan(steps, [0.5, seed / 20.0, 0.99], H0, W0, big)
        assert actions[0][0] == "crop" and actions[1] == ("flip", False) and params[4] == 0
        ex = P.apply_labels(dict(groundtruth_boxes=big, groundtruth_classes=np.eye(1, dtype=F)), actions)
        assert ex["groundtruth_boxes"].shape == (0, 4) and ex["groundtruth_classes"].shape == (0, 1)
    with pytest.raises(ValueError, match="needs the boxes"):
        P.plan(steps, [0.5, 0.5, 0.5], H0, W0, 1)
    # random_coef 1 keeps the original: the identity crop, no label action, boxes untouched (not even clipped)
    steps = P.parse_options(_opts(["random_crop_image { random_coef: 1 }"]), geometric=True)
    params, actions, frame = P.plan(steps, [0.3, 0.7], H0, W0, big, frame=True)
    assert list(params) == [0, 0, H0, W0] and actions == [] and frame == (H0, W0)


# ------------------------------------------------------------------------------ draws and gating
def test_draw_counts_are_fixed():
    opts = _opts(["random_crop_image { random_coef: 0 }", "random_pad_image { max_image_height: 1 max_image_width: 1 }",
                  "random_crop_pad_image { }", "ssd_random_crop { }",
                  "ssd_random_crop { operations { min_area: 0.5 max_area: 1 min_aspect_ratio: 1 max_aspect_ratio: 1 } }"])
    assert IP.option_draw_counts(opts, geometric=True) == [2, 4, 6, 3, 3]
    steps = P.parse_options(opts, geometric=True)
    assert P.program(steps) == [P.OP_CROP, P.OP_PAD, P.OP_CROP, P.OP_PAD, P.OP_CROP, P.OP_CROP]
    for boxes in (BOXES, np.zeros((0, 4), F)):
        params, _ = P.plan(steps, np.random.RandomState(0).uniform(size=18), H0, W0, boxes)
        assert params.size == P.num_params(P.program(steps)) == 4 + 8 + 12 + 4 + 4
    with pytest.raises(ValueError, match="17 draws for options that take 18"):
        P.plan(steps, [0.5] * 17, H0, W0, BOXES)
    assert len(steps[3].args["operations"]) == 7 and len(steps[4].args["operations"]) == 1


@pytest.mark.parametrize("opts", [["random_horizontal_flip { }"],
                                  ["normalize_image { original_maxval: 255 }", "random_distort_color { }",
                                   "random_black_patches { max_black_patches: 2 }", "random_jitter_boxes { }"]])
def test_other_configs_draw_and_compute_as_before(opts):
    opts = _opts(opts)
    assert IP.option_draw_counts(opts, geometric=True) == IP.option_draw_counts(opts)
    img = np.random.RandomState(0).randint(0, 256, (9, 11, 3)).astype(F)
    ex = dict(image=img, groundtruth_boxes=BOXES, window_boxes=BOXES[:1], groundtruth_edgemask=np.zeros((2, 4, 5), F))
    r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
    a, b = P.preprocess(ex, opts, r1), P.preprocess(ex, opts, r2, geometric=True)
    assert r1.uniform() == r2.uniform()
    np.testing.assert_array_equal(a["image"], b["image"])
    np.testing.assert_array_equal(a["groundtruth_boxes"], b["groundtruth_boxes"])
    assert "window_boxes" in a and not any(f in b for f in P.AUX_FIELDS)      # geometric mode drops the frozen labels


def test_gating():
    for kind in GEO:
        for call in (lambda: P.parse_options([kind]), lambda: IP.option_draw_counts([kind]),
                     lambda: IP.InputPipeline([], 3, 1, augmentation_options=[kind], num_workers=1),
                     lambda: next(R.batches([], 3, 1, [kind]), None) or P.preprocess(
                         dict(image=np.zeros((4, 4, 3), F), groundtruth_boxes=BOXES), [kind])):
            with pytest.raises(ValueError, match="not supported: .*old frame.*generate"):
                call()
        assert P.parse_options([kind], geometric=True)[0].kind == kind
    for kind, why in (("random_crop_to_aspect_ratio", "old frame"), ("ssd_random_crop_pad", "old frame"),
                      ("ssd_random_crop_fixed_aspect_ratio", "old frame"), ("random_image_scale", "resize_to_range"),
                      ("resize_image", "resize_to_range"), ("scale_boxes_to_pixel_coordinates", "normalised boxes")):
        with pytest.raises(ValueError, match="not supported: .*" + why) as e:
            P.parse_options([kind], geometric=True)
        assert "generate" not in str(e.value)


@pytest.mark.parametrize("text,field", [("min_area: 0", "min_area"), ("min_area: 0.6 max_area: 0.5", "min_area"),
                                        ("max_area: 1.5", "max_area"), ("min_aspect_ratio: 0", "min_aspect_ratio"),
                                        ("min_aspect_ratio: 2 max_aspect_ratio: 1", "max_aspect_ratio"),
                                        ("min_object_covered: 1.1", "min_object_covered"),
                                        ("overlap_thresh: -0.1", "overlap_thresh"), ("random_coef: 2", "random_coef")])
def test_bad_crop_arguments_name_the_field(text, field):
    for kind in ("random_crop_image", "random_crop_pad_image"):
        with pytest.raises(ValueError, match=r"%s: %s = " % (kind, field)):
            P.parse_options(_opts(["%s { %s }" % (kind, text)]), geometric=True)
    ok = "min_area: 0.1 max_area: 1 min_aspect_ratio: 0.5 max_aspect_ratio: 2 "
    with pytest.raises(ValueError, match=r"ssd_random_crop: operations\[1\]: %s = " % field):
        P.parse_options(_opts(["ssd_random_crop { operations { %s } operations { %s %s } }" % (ok, ok, text)]),
                        geometric=True)


def test_train_time_rule():
    model = lambda heads: config.parse_pipeline_config("model { faster_rcnn { } mtl { %s } }" % heads).model
    crop, flip = _opts(["random_horizontal_flip { }", "ssd_random_crop { }"]), _opts(["random_horizontal_flip { }"])
    with pytest.raises(ValueError, match=r"'ssd_random_crop' moves .*mtl\.window / mtl\.edgemask .*--aux_labels=generate"):
        train.geometric_augmentation(crop, model("window: true edgemask: true"), "record")
    assert train.geometric_augmentation(crop, model("window: true edgemask: true"), "generate") is True
    assert train.geometric_augmentation(crop, model("refine: true"), "record") is True       # no head reads frozen labels
    assert train.geometric_augmentation(flip, model("closeness: true"), "record") is False    # and nothing is refused


def test_descriptors_with_the_source_sizes_as_frames_are_those_without_frames():
    """What lets the pipeline pass every program's final frames: a program that moves no frame ends in the source size."""
    from mtl_ssl_amd import ops
    shapes, flips = [(37, 53), (64, 40), (33, 33)], [True, False, True]
    for OH, OW in ((24, 40), (37, 53)):
        plain, n = ops.image_descs(shapes, flips, OH, OW)
        framed, m = ops.image_descs(shapes, flips, OH, OW, frames=shapes)
        assert n == m == sum(h * w * 3 for h, w in shapes)
        assert plain.tobytes() == framed.tobytes()


# ------------------------------------------------------------------------------ the two feeds
K = 3
SHAPES = [(40, 56), (56, 40), (33, 33), (40, 56), (56, 40), (33, 33)]
FEED_OPTIONS = ["normalize_image { original_minval: 0 original_maxval: 255 target_minval: 0 target_maxval: 1 }",
                "random_crop_pad_image { min_object_covered: 0.5 }", "random_horizontal_flip { }",
                "random_distort_color { }",
                "normalize_image { original_minval: 0 original_maxval: 1 target_minval: 0 target_maxval: 255 }"]


def write_records(path, rng=None):
    """6 PNG records of three sizes, one of them without boxes, with frozen auxiliary labels that geometric mode drops."""
    from PIL import Image
    rng = rng or np.random.RandomState(4)
    recs = []
    for i, (h, w) in enumerate(SHAPES):
        buf = io.BytesIO()
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(buf, format="PNG")
        G = 0 if i == 2 else int(rng.randint(1, 4))
        y0, x0 = rng.uniform(0, 0.5, G).astype(F), rng.uniform(0, 0.5, G).astype(F)
        y1, x1 = (y0 + rng.uniform(0.2, 0.5, G)).astype(F), (x0 + rng.uniform(0.2, 0.5, G)).astype(F)
        recs.append(R.serialize_example({
            "image/encoded": buf.getvalue(), "image/format": b"png", "image/filename": "im%d.png" % i,
            "image/source_id": str(i), "image/height": np.array([h]), "image/width": np.array([w]),
            "image/object/bbox/ymin": y0, "image/object/bbox/xmin": x0, "image/object/bbox/ymax": y1,
            "image/object/bbox/xmax": x1, "image/object/class/label": rng.randint(1, K + 1, G).astype(np.int64),
            "image/object/difficult": rng.randint(0, 2, G).astype(np.int64),
            "image/edgemask/masks": rng.rand(2 * 4 * 5).astype(F), "image/edgemask/height": np.array([4]),
            "image/edgemask/width": np.array([5])}))
    R.write_tfrecord(path, recs)
    return path


def resized(h, w):
    s = 24.0 / min(h, w)
    if round(max(h, w) * s) > 40:
        s = 40.0 / max(h, w)
    return int(round(h * s)), int(round(w * s))


def assert_same_batches(got, want):
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert list(g) == list(w) and "groundtruth_edgemask" not in g
        np.testing.assert_array_equal(g["images"].cpu().numpy(), w["images"].cpu().numpy())
        for k in w:
            if k == "images":
                continue
            assert len(g[k]) == len(w[k])
            for a, b in zip(g[k], w[k]):
                if isinstance(b, str):
                    assert a == b
                else:
                    assert a.dtype == b.dtype
                    np.testing.assert_array_equal(a, b)


def test_the_two_feeds_yield_identical_batches(tmp_path):
    rec = write_records(str(tmp_path / "geo.record"))
    opts = _opts(FEED_OPTIONS)
    kw = dict(rng=None, resized_shape=resized, max_pending=4, geometric=True)
    want = list(R.batches([rec], K, 2, opts, **dict(kw, rng=np.random.RandomState(9))))
    with IP.InputPipeline([rec], K, 2, opts, device="cpu", num_workers=2, **dict(kw, rng=np.random.RandomState(9))) as pipe:
        got = list(pipe)
    assert_same_batches(got, want)
    shapes = {tuple(b["images"].shape[1:3]) for b in want}
    assert len(shapes) > 1                                          # bucketed by the final frames, which differ
    assert sum(len(b["groundtruth_boxes"]) for b in want) == len(SHAPES)
    for b in want:
        for boxes, classes, diff in zip(b["groundtruth_boxes"], b["groundtruth_classes"], b["groundtruth_difficult"]):
            assert len(boxes) == len(classes) == len(diff)
