"""CPU tests of the asynchronous input pipeline (mtl_ssl_amd/input_pipeline.py) with its host preparer: the batches
must equal input_reader.batches(...) for the same arguments, bit for bit and in the same order (record sharding,
the shuffle buffer, the flip draws, shape bucketing, max_pending flushes and the remainder), whatever the number of
decode workers; a corrupt record must surface in the consumer with its name and leave no child process behind."""
import io
import multiprocessing
import os

import numpy as np
import pytest

from mtl_ssl_amd import config
from mtl_ssl_amd import input_pipeline as P
from mtl_ssl_amd import input_reader as R

K = 3
SHAPES = [(12, 16), (16, 12), (20, 30), (30, 20), (9, 13), (13, 9), (16, 12), (12, 16), (25, 25), (7, 11), (20, 30)]
FLIP = config.parse_pipeline_config(
    "train_config { data_augmentation_options { random_horizontal_flip { } } }").train_config.data_augmentation_options
FLIP2 = FLIP + FLIP


def _png(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG")
    return b.getvalue()


def _example(rng, i, h, w, boxes=True):
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    G = int(rng.randint(1, 4)) if boxes else 0
    y0, x0 = rng.uniform(0, 0.5, G).astype(np.float32), rng.uniform(0, 0.5, G).astype(np.float32)
    y1, x1 = (y0 + rng.uniform(0.1, 0.5, G)).astype(np.float32), (x0 + rng.uniform(0.1, 0.5, G)).astype(np.float32)
    em = rng.rand(2, 4, 5).astype(np.float32)
    return R.serialize_example({
        "image/encoded": _png(img), "image/format": b"png", "image/filename": "im%d.png" % i,
        "image/source_id": str(i), "image/height": np.array([h]), "image/width": np.array([w]),
        "image/object/bbox/ymin": y0, "image/object/bbox/xmin": x0, "image/object/bbox/ymax": y1,
        "image/object/bbox/xmax": x1, "image/object/class/label": rng.randint(1, K + 1, G).astype(np.int64),
        "image/object/difficult": rng.randint(0, 2, G).astype(np.int64),
        "image/window/bbox/ymin": np.array([0.1], np.float32), "image/window/bbox/xmin": np.array([0.13], np.float32),
        "image/window/bbox/ymax": np.array([0.9], np.float32), "image/window/bbox/xmax": np.array([0.71], np.float32),
        "image/window/labels/text": [b"0.5 0.25 0 0.25"],
        "image/object/closeness/text": [b"0 1 0 0"] * G,
        "image/edgemask/masks": em.reshape(-1), "image/edgemask/height": np.array([4]),
        "image/edgemask/width": np.array([5])})


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    d = tmp_path_factory.mktemp("pipe")
    rng = np.random.RandomState(3)
    paths = []
    for part, shapes in enumerate((SHAPES[:6], SHAPES[6:])):
        p = str(d / ("part%d.record" % part))
        R.write_tfrecord(p, [_example(rng, 10 * part + i, h, w, boxes=(i != 2)) for i, (h, w) in enumerate(shapes)])
        paths.append(p)
    return paths


def _resized(h, w):
    """keep_aspect_ratio_resizer(min 18, max 28): upscales the small images, downscales the large ones."""
    s = 18.0 / min(h, w)
    if round(max(h, w) * s) > 28:
        s = 28.0 / max(h, w)
    return int(round(h * s)), int(round(w * s))


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w)
        assert g["images"].dtype == w["images"].dtype and np.array_equal(g["images"].numpy(), w["images"].numpy())
        for k in w:
            if k == "images":
                continue
            assert len(g[k]) == len(w[k]), k
            for a, b in zip(g[k], w[k]):
                if isinstance(b, str):
                    assert a == b, k
                else:
                    assert a.dtype == b.dtype and np.array_equal(a, b), k


def _both(paths, n_batches=None, workers=2, **kw):
    seed = kw.pop("seed", 7)
    ref = R.batches(paths, K, rng=np.random.RandomState(seed), **kw)
    with P.InputPipeline(paths, K, rng=np.random.RandomState(seed), num_workers=workers, prefetch=2, **kw) as pipe:
        if n_batches is None:
            return list(pipe), list(ref)
        return [next(pipe) for _ in range(n_batches)], [next(ref) for _ in range(n_batches)]


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("drop", [False, True])
def test_batches_equal_the_host_generator(records, B, drop):
    got, want = _both(records, batch_size=B, augmentation_options=FLIP, resized_shape=_resized, max_pending=3,
                      drop_remainder=drop)
    _assert_same(got, want)
    assert sum(len(b["filename"]) for b in want) <= len(SHAPES)


def test_own_shapes_without_a_resizer(records):
    got, want = _both(records, batch_size=2, augmentation_options=FLIP2)
    _assert_same(got, want)
    assert {tuple(b["images"].shape[1:3]) for b in got} >= {(12, 16), (16, 12)}


@pytest.mark.parametrize("rank", [0, 1])
def test_shuffle_buffer_flip_and_ranks(records, rank):
    got, want = _both(records, batch_size=2, augmentation_options=FLIP2, resized_shape=_resized, shuffle_buffer=4,
                      rank=rank, world=2, max_pending=4)
    _assert_same(got, want)
    names = [n for b in got for n in b["filename"]]
    assert len(names) == len(set(names))


def test_loop_over_more_than_one_epoch(records):
    got, want = _both(records, n_batches=14, batch_size=2, augmentation_options=FLIP, resized_shape=_resized,
                      shuffle_buffer=3, loop=True, max_pending=5)
    _assert_same(got, want)
    assert sum(len(b["filename"]) for b in got) > len(SHAPES)


def test_worker_count_does_not_change_the_sequence(records):
    kw = dict(batch_size=2, augmentation_options=FLIP, resized_shape=_resized, shuffle_buffer=5, max_pending=4)
    one, want = _both(records, workers=1, **kw)
    three, _ = _both(records, workers=3, **kw)
    _assert_same(one, want)
    _assert_same(three, want)


def test_default_worker_count_follows_the_affinity_mask():
    cpus = len(os.sched_getaffinity(0))
    assert P.default_num_workers(8, 1) == max(1, min(8, cpus - 1))
    assert P.default_num_workers(64, 1000) == 1


def test_corrupt_record_names_itself_and_leaves_no_children(records, tmp_path):
    rng = np.random.RandomState(1)
    recs = [_example(rng, i, 12, 16) for i in range(4)]
    recs[2] = R.serialize_example({"image/encoded": b"not an image", "image/filename": "bad.png"})
    p = str(tmp_path / "bad.record")
    R.write_tfrecord(p, recs)
    pipe = P.InputPipeline([p], K, 1, num_workers=2)
    procs = list(pipe._procs)
    assert procs and all(pr.is_alive() for pr in procs)
    with pytest.raises(P.InputPipelineError, match=r"record 2 of .*bad\.record"):
        list(pipe)
    assert not any(pr.is_alive() for pr in procs)
    assert not multiprocessing.active_children()


def test_unsupported_augmentation_is_refused():
    with pytest.raises(ValueError, match="not supported"):
        P.InputPipeline([], K, 1, augmentation_options=["random_crop"], num_workers=1)
