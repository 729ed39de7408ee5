"""Photometric programs on the GPU: mtlssl_prepare_images_aug, the one program evaluator, against the host restatement
resize_bilinear_legacy(preprocessor.apply_program(float32(img))) bit for bit (each op alone, chains with flips around
the position-dependent ops, two contrast ops, both random_distort_color orderings, odd sizes, the no-resize case,
up to 8 images per launch), the empty program against mtlssl_prepare_images, the pipeline's device batches against
input_reader.batches on a busy stream, and the train launcher with either feed.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage, after every kernel-parity module."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TO_UNIT = {"normalize_image": {"original_minval": 0.0, "original_maxval": 255.0, "target_minval": 0.0,
                               "target_maxval": 1.0}}
TO_255 = {"normalize_image": {"original_minval": 0.0, "original_maxval": 1.0, "target_minval": 0.0,
                              "target_maxval": 255.0}}
FLIP = {"random_horizontal_flip": {}}
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


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    return ops


def _params(steps, rng, shapes):
    from mtl_ssl_amd import preprocessor as P
    return [P.plan(steps, rng.uniform(size=P.draw_count(steps)), h, w, 1)[0] for h, w in shapes]


def _device(ops, imgs, codes, params, OH, OW, flips=None):
    desc, nbytes = ops.image_descs([a.shape[:2] for a in imgs], flips or [False] * len(imgs), OH, OW)
    dev = torch.device("cuda")
    d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    p = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    P = len(params[0]) if params else 0
    prm = torch.from_numpy(np.stack(params).astype(np.float32) if P else np.zeros((1,), np.float32)).to(dev)
    return ops.prepare_images_aug(p, d, len(imgs), OH, OW, codes, prm, P, max(a.shape[0] for a in imgs)).cpu().numpy()


def _check(ops, options, shapes, targets, seed):
    from mtl_ssl_amd import preprocessor as P
    rng = np.random.RandomState(seed)
    steps = P.parse_options(options, warn=False)
    codes = P.program(steps)
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    params = _params(steps, rng, shapes)
    for OH, OW in targets:
        got = _device(ops, imgs, codes, params, OH, OW)
        for i, img in enumerate(imgs):
            want = P.resize_bilinear_legacy(P.apply_program(img.astype(np.float32), codes, params[i]), OH, OW)
            np.testing.assert_array_equal(got[i], want, err_msg="%s image %d -> %s" % (options, i, (OH, OW)))


SINGLE = [
    [TO_UNIT], [{"subtract_channel_mean": {"means": [120.5, 99.25, 7.0]}}],
    [TO_UNIT, {"random_adjust_brightness": {}}], [TO_UNIT, {"random_adjust_contrast": {}}],
    [TO_UNIT, {"random_adjust_saturation": {"min_delta": 0.0, "max_delta": 2.0}}],
    [TO_UNIT, {"random_adjust_hue": {"max_delta": 0.5}}], [{"random_adjust_hue": {}}],
    [TO_UNIT, {"random_distort_color": {"color_ordering": 0}}], [TO_UNIT, {"random_distort_color": {"color_ordering": 1}}],
    [{"random_rgb_to_gray": {"probability": 1.0}}], [TO_UNIT, {"random_pixel_value_scale": {}}],
    [{"random_black_patches": {"max_black_patches": 5, "probability": 1.0, "size_to_image_ratio": 0.3}}],
    [{"random_jitter_boxes": {}}], [FLIP],
]


@pytest.mark.parametrize("case", range(len(SINGLE)))
def test_each_op_alone_matches_the_host(ops, case):
    _check(ops, SINGLE[case], [(31, 17), (7, 13), (48, 64)], [(31, 17), (45, 29), (5, 8)], 10 + case)


CHAINS = [
    [TO_UNIT, FLIP, {"random_black_patches": {"max_black_patches": 3, "probability": 1.0, "size_to_image_ratio": 0.25}},
     FLIP, {"random_pixel_value_scale": {}}, FLIP, {"random_adjust_contrast": {}}, TO_255],
    [TO_UNIT, {"random_adjust_contrast": {"min_delta": 0.3, "max_delta": 0.6}}, FLIP,
     {"random_adjust_contrast": {"min_delta": 1.5, "max_delta": 2.5}}, {"random_rgb_to_gray": {"probability": 0.5}}],
    [TO_UNIT, {"random_distort_color": {"color_ordering": 0}}, FLIP, {"random_distort_color": {"color_ordering": 1}},
     {"random_pixel_value_scale": {"minval": 0.5, "maxval": 1.5}}, TO_255],
]


@pytest.mark.parametrize("case", range(len(CHAINS)))
def test_chains_with_flips_match_the_host(ops, case):
    shapes = [(375, 500), (1, 9), (9, 1), (33, 47), (500, 333), (12, 12), (64, 48), (7, 13)]     # B = 8
    _check(ops, CHAINS[case], shapes, [(600, 800), (37, 23)], 40 + case)
    _check(ops, CHAINS[case], [(33, 47)], [(33, 47)], 50 + case)                                # no-resize case


def test_empty_program_equals_prepare_images(ops):
    rng = np.random.RandomState(3)
    shapes = [(375, 500), (7, 13), (1, 1), (480, 640)]
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    flips = [True, False, True, False]
    dev = torch.device("cuda")
    for OH, OW in ((600, 800), (7, 13), (33, 21)):
        desc, _ = ops.image_descs(shapes, flips, OH, OW)
        d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        p = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
        want = ops.prepare_images(p, d, len(imgs), OH, OW)
        got = ops.prepare_images_aug(p, d, len(imgs), OH, OW, [], torch.zeros(1, device=dev), 0, 480)
        assert torch.equal(got, want), (OH, OW)


def test_bad_programs_are_refused(ops):
    from mtl_ssl_amd.lib import MtlsslError
    img = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(MtlsslError, match="bad op code 99"):
        _device(ops, [img], [0, 99], [np.zeros(2, np.float32)], 4, 5)
    with pytest.raises(MtlsslError, match="bad op code 13"):          # the first code past OP_PAD
        _device(ops, [img], [13], [np.zeros(1, np.float32)], 4, 5)
    with pytest.raises(MtlsslError, match="takes 3 parameters per image, P = 2"):
        _device(ops, [img], [1], [np.zeros(2, np.float32)], 4, 5)


def _write_records(path, shapes, K, rng):
    from PIL import Image
    from mtl_ssl_amd import input_reader as R
    from mtl_ssl_amd import labels
    recs = []
    for i, (H, W) in enumerate(shapes):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        G = int(rng.randint(1, 4))
        cyx, hw = rng.uniform(0.25, 0.75, (G, 2)), rng.uniform(0.2, 0.5, (G, 2))
        b = np.concatenate([cyx - hw / 2, cyx + hw / 2], 1).clip(0, 1).astype(np.float32)
        cls = rng.randint(0, K, G)
        abs_b = b * [H, W, H, W]
        wb, wl = labels.random_windows(abs_b, cls + 1, W, H, K, rng, 6)
        clo = labels.closeness_labels(abs_b, cls + 1, W, H, K)
        em = labels.edgemask(abs_b, W, H).astype(np.float32)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=90)
        recs.append(R.serialize_example({
            "image/encoded": buf.getvalue(), "image/format": b"jpeg", "image/filename": "im%d.jpg" % i,
            "image/source_id": str(i), "image/height": np.array([H]), "image/width": np.array([W]),
            "image/object/bbox/ymin": b[:, 0], "image/object/bbox/xmin": b[:, 1],
            "image/object/bbox/ymax": b[:, 2], "image/object/bbox/xmax": b[:, 3],
            "image/object/class/label": (cls + 1).astype(np.int64), "image/object/difficult": np.zeros(G, np.int64),
            "image/window/bbox/ymin": wb[:, 0], "image/window/bbox/xmin": wb[:, 1],
            "image/window/bbox/ymax": wb[:, 2], "image/window/bbox/xmax": wb[:, 3],
            "image/window/labels/text": [" ".join("%.6f" % v for v in row).encode() for row in wl],
            "image/object/closeness/text": [" ".join("%.6f" % v for v in row).encode() for row in clo],
            "image/edgemask/masks": em.reshape(-1), "image/edgemask/height": np.array([em.shape[1]]),
            "image/edgemask/width": np.array([em.shape[2]])}))
    R.write_tfrecord(path, recs)


def test_pipeline_batches_with_every_option_equal_the_host_generator(ops, tmp_path):
    from mtl_ssl_amd import config, input_pipeline, input_reader
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
    K = 5
    rec = str(tmp_path / "voc.record")
    _write_records(rec, [(375, 500), (500, 375), (333, 500), (375, 500), (480, 640), (500, 375), (375, 500),
                         (427, 640), (500, 333)], K, np.random.RandomState(4))
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "frcnn_mobilenet_v1_voc_mtl.config")).read())
    rz = cfg.model.faster_rcnn.image_resizer
    opts = config.parse_pipeline_config(ALL_OPTIONS).train_config.data_augmentation_options
    kw = dict(augmentation_options=opts, loop=True, shuffle_buffer=3, max_pending=4,
              resized_shape=lambda h, w: M.resized_shape(h, w, rz))
    ref = input_reader.batches([rec], K, 2, rng=np.random.RandomState(9), **kw)
    dev = torch.device("cuda")
    a = torch.randn(2048, 2048, device=dev)
    with input_pipeline.InputPipeline([rec], K, 2, rng=np.random.RandomState(9), device=dev, num_workers=3,
                                      prefetch=3, **kw) as pipe:
        for step in range(6):
            for _ in range(4):
                a = torch.tanh(a @ a * 1e-3)          # the consumer's stream stays busy between hand-outs
            got, want = next(pipe), next(ref)
            assert list(got) == list(want)
            assert got["images"].is_cuda and torch.equal(got["images"].clone(), want["images"].to(dev)), step
            for k in want:
                if k != "images":
                    assert all((x == y) if isinstance(y, str) else np.array_equal(x, y)
                               for x, y in zip(got[k], want[k])), k
    torch.cuda.synchronize()


def test_train_launcher_writes_the_same_checkpoint_with_either_feed(tmp_path):
    import __graft_entry__ as g
    g.build()
    K = 5
    rec = str(tmp_path / "voc.record")
    _write_records(rec, [(160, 224), (224, 160), (150, 210), (160, 224), (200, 150), (160, 224)], K,
                   np.random.RandomState(5))
    text = open(os.path.join(ROOT, "configs", "smoke_resnet50_mtl.config")).read()
    text += ALL_OPTIONS
    text += 'train_input_reader { min_after_dequeue: 4 num_readers: 2 tf_record_input_reader { input_path: "%s" } }\n' % rec
    cfgp = str(tmp_path / "pipeline.config")
    open(cfgp, "w").write(text)
    env = dict(os.environ, PYTHONPATH=ROOT)
    runs = {}
    for feed in ("host", "async"):
        run = str(tmp_path / ("run_" + feed))
        r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.train", "--train_dir=" + run, "--pipeline_config_path=" + cfgp,
                            "--num_steps=3", "--input_pipeline=" + feed], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[feed] = dict(np.load(os.path.join(run, "model.ckpt.npz")))
    assert sorted(runs["host"]) == sorted(runs["async"])
    for k, v in runs["host"].items():
        assert np.array_equal(v, runs["async"][k]), k
