"""mtlssl_prepare_images_aug with crop / pad ops inside the device image preparation against the host restatement
resize_bilinear_legacy(apply_program(...)), bit for bit: B = 3 sources of 37x53, 64x40 and 33x33 with parameters from
plan() on fixed draws, every program once with a resize to 24 x 40 and once with the output equal to the final frame
(the no-resize branch); a program without geometric ops must give the same output with and without its frames."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(37, 53), (64, 40), (33, 33)]
BOXES = np.float32([[0.1, 0.1, 0.6, 0.5], [0.3, 0.4, 0.9, 0.9]])
TO_UNIT = "normalize_image { original_minval: 0 original_maxval: 255 target_minval: 0 target_maxval: 1 }"
TO_255 = "normalize_image { original_minval: 0 original_maxval: 1 target_minval: 0 target_maxval: 255 }"
SCALE, PATCH = "random_pixel_value_scale { }", "random_black_patches { max_black_patches: 3 probability: 0.8 size_to_image_ratio: 0.3 }"
PROGRAMS = {
    "crop": ["random_crop_image { min_object_covered: 0.3 }"],
    "identity_crop": ["random_crop_image { random_coef: 1 }"],
    "pad_given_colour": ["random_pad_image { pad_color: [7.5, 120, 250] }"],
    "pad_mean_colour": ["random_pad_image { }"],
    "crop_pad": ["random_crop_pad_image { min_object_covered: 0.3 }"],
    "pad_crop_into_the_padding": ["random_pad_image { }", "random_crop_image { min_object_covered: 0 min_area: 0.5 }"],
    "flip_between": ["ssd_random_crop { }", "random_horizontal_flip { }", "random_pad_image { pad_color: [1, 2, 3] }",
                     "random_horizontal_flip { }", "random_crop_image { min_object_covered: 0 }"],
    "crop_meanpad_contrast": [TO_UNIT, "random_crop_pad_image { min_object_covered: 0.3 }", "random_adjust_contrast { }",
                              TO_255],
    "position_ops_around_a_crop": [TO_UNIT, SCALE, PATCH, "random_crop_image { min_object_covered: 0.3 }", SCALE, PATCH,
                                   TO_255],
}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    return ops


def _options(text):
    from mtl_ssl_amd import config
    return config.parse_pipeline_config("train_config { %s }" % " ".join(
        "data_augmentation_options { %s }" % t for t in text)).train_config.data_augmentation_options


def _planned(name, seed=11):
    """-> (codes, uint8 images, per-image parameters, final frames, per-image tallest stage frame)."""
    from mtl_ssl_amd import preprocessor as P
    steps = P.parse_options(_options(PROGRAMS[name]), warn=False, geometric=True)
    codes = P.program(steps)
    rng = np.random.RandomState(seed)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    params, frames, tallest = [], [], []
    for h, w in SHAPES:
        p, _, frame = P.plan(steps, rng.uniform(size=P.draw_count(steps)), h, w, BOXES, frame=True)
        params.append(p)
        frames.append(frame)
        tallest.append(max(fh for fh, _ in P.stage_frames(codes, p, h, w)))
    return codes, imgs, params, frames, tallest


def _device(ops, imgs, codes, params, OH, OW, frames, max_H):
    desc, _ = ops.image_descs([a.shape[:2] for a in imgs], [False] * len(imgs), OH, OW, frames)
    dev = torch.device("cuda")
    d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    px = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    n = len(params[0])
    prm = torch.from_numpy(np.stack(params).astype(np.float32) if n else np.zeros((1,), np.float32)).to(dev)
    return ops.prepare_images_aug(px, d, len(imgs), OH, OW, codes, prm, n, max_H).cpu().numpy()


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_geo_matches_the_host_restatement(ops, name):
    from mtl_ssl_amd import preprocessor as P
    codes, imgs, params, frames, tallest = _planned(name)
    host = [P.apply_program(np.float32(a), codes, p) for a, p in zip(imgs, params)]
    assert [h.shape[:2] for h in host] == frames
    if name == "identity_crop":
        assert frames == SHAPES
    if name == "pad_crop_into_the_padding":      # some crop holds pixels of the padding and pixels of the image
        hit = 0
        for (h, w), p in zip(SHAPES, params):
            oy, ox = int(p[0]), int(p[1])
            y0, x0, ch, cw = (int(v) for v in p[8:12])
            inside = max(0, min(y0 + ch, oy + h) - max(y0, oy)) * max(0, min(x0 + cw, ox + w) - max(x0, ox))
            hit += 0 < inside < ch * cw
        assert hit
    if name == "flip_between":
        assert any(p[4] != 0 for p in params) and any(p[13] != 0 for p in params)
    # one launch for the three images, resized
    OH, OW = 24, 40
    got = _device(ops, imgs, codes, params, OH, OW, frames, max(tallest))
    for i, h in enumerate(host):
        np.testing.assert_array_equal(got[i], P.resize_bilinear_legacy(h, OH, OW), err_msg="%s image %d" % (name, i))
    # the no-resize branch: the output is the final frame
    for i, h in enumerate(host):
        got = _device(ops, imgs[i:i + 1], codes, params[i:i + 1], frames[i][0], frames[i][1], frames[i:i + 1],
                      tallest[i])
        np.testing.assert_array_equal(got[0], h, err_msg="%s image %d unresized" % (name, i))


def test_a_program_without_geometric_ops_equals_prepare_images_aug(ops):
    from mtl_ssl_amd import preprocessor as P
    text = [TO_UNIT, "random_horizontal_flip { }", "random_adjust_contrast { }", SCALE, "random_adjust_hue { }", PATCH,
            "random_distort_color { color_ordering: 1 }", "random_horizontal_flip { }", TO_255]
    steps = P.parse_options(_options(text), warn=False)
    codes = P.program(steps)
    rng = np.random.RandomState(5)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    params = [P.plan(steps, rng.uniform(size=P.draw_count(steps)), h, w, BOXES)[0] for h, w in SHAPES]
    assert any(p[3] != 0 for p in params)
    max_H = max(h for h, _ in SHAPES)
    host = [P.apply_program(np.float32(a), codes, p) for a, p in zip(imgs, params)]
    for OH, OW in ((24, 40), (37, 53)):          # at 37 x 53 image 0 takes the no-resize branch, the other two are resized
        got = _device(ops, imgs, codes, params, OH, OW, None, max_H)
        for i, h in enumerate(host):
            np.testing.assert_array_equal(got[i], P.resize_bilinear_legacy(h, OH, OW), err_msg="image %d -> %d" % (i, OH))
        np.testing.assert_array_equal(_device(ops, imgs, codes, params, OH, OW, SHAPES, max_H), got)
