"""The asynchronous input pipeline on the GPU: mtlssl_prepare_images against the host expression
resize_bilinear_legacy(flip(float32(img))) bit for bit, the pipeline's device batches against input_reader.batches
while the consumer's stream is busy, and both launchers with --input_pipeline=host against the default.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage (records -> launchers), after every kernel-parity module."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    return ops


def _host(img, flip, OH, OW):
    from mtl_ssl_amd import preprocessor
    x = np.asarray(img, np.float32)
    if flip:
        x = x[:, ::-1].copy()
    return preprocessor.resize_bilinear_legacy(x, OH, OW)


def _device(ops, imgs, flips, OH, OW):
    desc, nbytes = ops.image_descs([a.shape[:2] for a in imgs], flips, OH, OW)
    pixels = np.concatenate([a.reshape(-1) for a in imgs]) if imgs else np.zeros(0, np.uint8)
    assert pixels.size == nbytes
    dev = torch.device("cuda")
    d = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    p = torch.from_numpy(pixels).to(dev)
    return ops.prepare_images(p, d, len(imgs), OH, OW).cpu()


def _resizer(name):
    from mtl_ssl_amd import config
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", name)).read())
    return cfg.model.faster_rcnn.image_resizer


SOURCES = [(1, 1), (1, 9), (9, 1), (7, 13), (31, 17), (375, 500), (500, 333), (480, 640), (427, 640)]


def test_prepare_images_matches_the_host_expression(ops):
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
    rng = np.random.RandomState(0)
    targets = {"identity": None, "small": (5, 8), "up": (45, 29)}
    for cfg in ("frcnn_resnet101_coco_mtl.config", "frcnn_mobilenet_v1_voc_mtl.config"):
        rz = _resizer(cfg)
        targets[cfg] = rz
    n = 0
    for h, w in SOURCES:
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        for name, t in targets.items():
            if t is None:
                OH, OW = h, w
            elif isinstance(t, tuple):
                OH, OW = t
            else:
                OH, OW = M.resized_shape(h, w, t)
            for flip in (False, True):
                got = _device(ops, [img], [flip], OH, OW)[0]
                want = torch.from_numpy(_host(img, flip, OH, OW))
                assert torch.equal(got, want), (h, w, OH, OW, flip, float((got - want).abs().max()))
                n += 1
    assert n == len(SOURCES) * len(targets) * 2


def test_prepare_images_several_sizes_in_one_launch(ops):
    rng = np.random.RandomState(1)
    shapes = [(375, 500), (480, 640), (7, 13), (500, 333)]
    imgs = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    flips = [True, False, True, False]
    for OH, OW in ((600, 800), (375, 500), (33, 21)):
        got = _device(ops, imgs, flips, OH, OW)
        for i, (img, f) in enumerate(zip(imgs, flips)):
            assert torch.equal(got[i], torch.from_numpy(_host(img, f, OH, OW))), (i, OH, OW)


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


def test_pipeline_batches_equal_the_host_generator_on_a_busy_stream(ops, tmp_path):
    from mtl_ssl_amd import config, input_pipeline, input_reader
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
    K = 5
    rec = str(tmp_path / "voc.record")
    _write_records(rec, [(375, 500), (500, 375), (333, 500), (375, 500), (480, 640), (500, 375), (375, 500),
                         (427, 640), (500, 333)], K, np.random.RandomState(4))
    rz = _resizer("frcnn_mobilenet_v1_voc_mtl.config")
    opts = config.parse_pipeline_config("train_config { data_augmentation_options { random_horizontal_flip { } } }"
                                        ).train_config.data_augmentation_options
    kw = dict(augmentation_options=opts, loop=True, shuffle_buffer=3, max_pending=4,
              resized_shape=lambda h, w: M.resized_shape(h, w, rz))
    ref = input_reader.batches([rec], K, 2, rng=np.random.RandomState(9), **kw)
    dev = torch.device("cuda")
    a = torch.randn(2048, 2048, device=dev)
    with input_pipeline.InputPipeline([rec], K, 2, rng=np.random.RandomState(9), device=dev, num_workers=3,
                                      prefetch=3, **kw) as pipe:
        for step in range(8):
            for _ in range(4):
                a = torch.tanh(a @ a * 1e-3)          # the consumer's stream stays busy between hand-outs
            got, want = next(pipe), next(ref)
            assert list(got) == list(want)
            assert got["images"].is_cuda and torch.equal(got["images"].clone(), want["images"].to(dev)), step
            for k in want:
                if k != "images":
                    assert all((x == y) if isinstance(y, str) else np.array_equal(x, y)
                               for x, y in zip(got[k], want[k])), k
        assert pipe.num_workers == 3
    torch.cuda.synchronize()


def test_launchers_give_the_same_results_with_either_feed(tmp_path):
    import __graft_entry__ as g
    g.build()
    K = 5
    rec = str(tmp_path / "voc.record")
    _write_records(rec, [(160, 224), (224, 160), (150, 210), (160, 224), (200, 150), (160, 224)], K,
                   np.random.RandomState(5))
    text = open(os.path.join(ROOT, "configs", "smoke_resnet50_mtl.config")).read()
    text += '\ntrain_config { data_augmentation_options { random_horizontal_flip { } } }\n'
    text += 'train_input_reader { min_after_dequeue: 4 num_readers: 2 tf_record_input_reader { input_path: "%s" } }\n' % rec
    text += 'eval_config { num_examples: 4 }\neval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % rec
    cfgp = str(tmp_path / "pipeline.config")
    open(cfgp, "w").write(text)
    env = dict(os.environ, PYTHONPATH=ROOT)
    runs, metrics = {}, {}
    for feed in ("host", "async"):
        run = str(tmp_path / ("run_" + feed))
        r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.train", "--train_dir=" + run, "--pipeline_config_path=" + cfgp,
                            "--num_steps=3", "--input_pipeline=" + feed], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[feed] = dict(np.load(os.path.join(run, "model.ckpt.npz")))
        ed = str(tmp_path / ("eval_" + feed))
        r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.eval", "--checkpoint_dir=" + str(tmp_path / "run_host"),
                            "--eval_dir=" + ed, "--pipeline_config_path=" + cfgp, "--input_pipeline=" + feed],
                           env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        metrics[feed] = open(os.path.join(ed, "metrics-3.json")).read()
    assert sorted(runs["host"]) == sorted(runs["async"])
    for k, v in runs["host"].items():
        assert np.array_equal(v, runs["async"][k]), k
    assert metrics["host"] == metrics["async"]
    assert json.loads(metrics["async"])["num_images"] == 4
