"""Host side of the generated auxiliary labels (Trainer(aux_labels="generate")): the unrounded definitions
labels.window_labels_exact / closeness_labels_exact / edgemask_exact against the rounded functions that
tests/test_host_logic.py pins to the reference, labels.draw_windows' distribution and determinism, and the launcher /
trainer switch. No GPU."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# round(v, 3) moves a value by at most half a unit of the third decimal; the golden file's pixel boxes pass through
# normalised float32 here (and closeness_labels returns float32), which moves a value by ~1e-7 more
HALF_UNIT = 5e-4 + 1e-6


def _gold():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "aux_labels_golden.json")))["cases"]


def _norm(abs_boxes, H, W):
    b = np.asarray(abs_boxes, np.float64).reshape(-1, 4)
    return (b / [H, W, H, W]).astype(np.float32)


def _abs(norm, H, W):
    return np.asarray(norm, np.float32).astype(np.float64) * [H, W, H, W]


def _rounded_window_labels(labels, boxes, ids, windows, K, H, W):
    b = _abs(boxes, H, W)
    return np.stack([labels.window_label(b, ids, w, K)[0] for w in _abs(windows, H, W)])


def _random_case(rng):
    K = int(rng.choice([5, 20, 90]))
    H, W = int(rng.randint(200, 700)), int(rng.randint(200, 900))
    G = int(rng.randint(1, 41))
    cyx, hw = rng.uniform(0, 1, (G, 2)), rng.uniform(0.03, 0.7, (G, 2))
    boxes = np.concatenate([cyx - hw / 2, cyx + hw / 2], 1).clip(0, 1).astype(np.float32)
    boxes = boxes[(boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])]
    if not len(boxes):
        boxes = np.array([[0.25, 0.25, 0.75, 0.75]], np.float32)
    ids = rng.randint(1, min(K, 6) + 1, len(boxes))
    return K, H, W, boxes, ids


def test_exact_definitions_against_the_rounded_functions_on_the_golden_cases():
    from mtl_ssl_amd import labels
    diffs = []
    for c in _gold():
        K, W, H = c["K"], c["width"], c["height"]
        boxes, ids = _norm(c["boxes"], H, W), np.asarray(c["classes"], np.int64)
        windows = np.asarray(c["window_boxes"], np.float32)
        exact = labels.window_labels_exact(boxes, ids, windows, K, H, W)
        assert exact.shape == (len(windows), K + 1)
        np.testing.assert_allclose(exact.sum(1), 1.0, rtol=0, atol=1e-12)
        assert np.abs(exact - _rounded_window_labels(labels, boxes, ids, windows, K, H, W)).max() <= HALF_UNIT
        # the file's own labels come from the reference's inclusion-exclusion: a value on a rounding boundary may land
        # on the other side (tests/test_host_logic.py allows the same one unit on under 0.5 % of the entries)
        diffs.append(np.abs(exact - np.asarray(c["window_labels"])).ravel())
        if len(boxes):
            clo = labels.closeness_labels_exact(boxes, ids, K, H, W)
            assert np.abs(clo - labels.closeness_labels(_abs(boxes, H, W), ids, W, H, K)).max() <= HALF_UNIT
            cd = np.abs(clo - np.asarray(c["closeness"]))
            assert cd.max() <= 1.5e-3 and (cd <= HALF_UNIT).mean() >= 0.995
        em = labels.edgemask_exact(boxes, H, W)
        ref = labels.edgemask(_abs(boxes, H, W), W, H)
        assert em.dtype == np.float32 and em.shape == (2, 64, 64)
        np.testing.assert_array_equal(em[0], ref[0])
        np.testing.assert_allclose(em[1], ref[1], rtol=1e-6)
        np.testing.assert_array_equal(em[0].astype(int), np.asarray(c["edgemask_fg"]))
        np.testing.assert_allclose(em[1].astype(np.float64).sum(1), c["edgemask_weight_sum_rows"], rtol=1e-5)
        np.testing.assert_allclose(em[1].astype(np.float64)[::7, ::5], c["edgemask_weight_probe"], rtol=1e-5)
    d = np.concatenate(diffs)
    assert d.max() <= 1.5e-3 and (d <= HALF_UNIT).mean() >= 0.995, (d.max(), (d <= HALF_UNIT).mean())


def test_exact_definitions_against_the_rounded_functions_on_random_cases():
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(11)
    for n in range(300):
        K, H, W, boxes, ids = _random_case(rng)
        lo, size = rng.uniform(0, 0.6, (3, 2)), rng.uniform(0.1, 0.6, (3, 2))
        windows = np.concatenate([lo, np.minimum(lo + size, 1.0)], 1).astype(np.float32)
        windows = np.concatenate([windows, [[0, 0, 1, 1]]]).astype(np.float32)
        onehot = np.zeros((len(ids), K), np.float32)
        onehot[np.arange(len(ids)), ids - 1] = 1
        exact = labels.window_labels_exact(boxes, onehot, windows, K, H, W)          # classes as the trainer has them
        np.testing.assert_array_equal(exact, labels.window_labels_exact(boxes, ids, windows, K, H, W))
        assert np.abs(exact - _rounded_window_labels(labels, boxes, ids, windows, K, H, W)).max() <= HALF_UNIT, n
        clo = labels.closeness_labels_exact(boxes, onehot, K, H, W)
        assert np.abs(clo - labels.closeness_labels(_abs(boxes, H, W), ids, W, H, K)).max() <= HALF_UNIT, n
        em, ref = labels.edgemask_exact(boxes, H, W), labels.edgemask(_abs(boxes, H, W), W, H)
        np.testing.assert_array_equal(em[0], ref[0])
        np.testing.assert_allclose(em[1], ref[1], rtol=1e-6)
    one = labels.closeness_labels_exact(boxes[:1], ids[:1], K, H, W)
    assert one.shape == (1, K + 1) and one[0, 0] == 1 and one[0, 1:].sum() == 0
    same = labels.closeness_labels_exact(boxes[:1].repeat(3, 0), [2, 2, 2], K, H, W)
    assert (same[:, 0] == 1).all() and same[:, 1:].sum() == 0


def _boxes_for_windows(rng, G):
    """Boxes that cover at least 5 % of the image, so that a redrawn window meets one within a few attempts."""
    cyx = rng.uniform(0.3, 0.7, (G, 2))
    hw = rng.uniform(0.25, 0.5, (G, 2))
    return np.concatenate([cyx - hw / 2, cyx + hw / 2], 1).clip(0, 1).astype(np.float32)


def test_draw_windows_distribution_and_determinism():
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(3)
    for H, W, G in ((375, 500, 3), (600, 1024, 1), (160, 224, 7), (48, 36, 2)):
        boxes = _boxes_for_windows(rng, G)
        assert ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).max() >= 0.05
        wins, attempts = labels.draw_windows(boxes, H, W, 64, seed=5, step=2, image=1, return_attempts=True)
        assert wins.dtype == np.float32 and wins.shape == (64, 4)
        assert attempts.max() < labels.WINDOW_ATTEMPTS          # no slot came out by the "keep the last draw" escape
        assert (wins >= 0).all() and (wins <= 1).all()
        hpx = (wins[:, 2].astype(np.float64) - wins[:, 0]) * H
        wpx = (wins[:, 3].astype(np.float64) - wins[:, 1]) * W
        assert (hpx >= min(32.0, H) - 1e-3).all() and (wpx >= min(32.0, W) - 1e-3).all()
        b, w = _abs(boxes, H, W), _abs(wins, H, W)
        for y0, x0, y1, x1 in w:                                 # every window meets an object
            assert ((np.minimum(y1, b[:, 2]) > np.maximum(y0, b[:, 0])) & (np.minimum(x1, b[:, 3]) > np.maximum(x0, b[:, 1]))).any()
        np.testing.assert_array_equal(wins, labels.draw_windows(boxes, H, W, 64, seed=5, step=2, image=1))
        for other in (dict(seed=5, step=3, image=1), dict(seed=5, step=2, image=0), dict(seed=6, step=2, image=1)):
            assert not np.array_equal(wins, labels.draw_windows(boxes, H, W, 64, **other))
        if min(H, W) >= 100:                                     # (in a 36-px image the fix-ups make windows coincide)
            assert len({tuple(r) for r in wins.tolist()}) == 64  # slots are independent draws
        np.testing.assert_array_equal(wins[:8], labels.draw_windows(boxes, H, W, 8, seed=5, step=2, image=1))
    # the sizes follow create_multi_object: uniform in [min_obj_size, side] before clipping, so the mean clipped height
    # is well inside (0.2, 0.6) of the image
    wins = labels.draw_windows(_boxes_for_windows(rng, 4), 480, 640, 2000, seed=1, step=0, image=0)
    assert 0.2 < float((wins[:, 2] - wins[:, 0]).mean()) < 0.6


def test_draw_windows_empty_image_repeats_its_first_window():
    from mtl_ssl_amd import labels
    wins, attempts = labels.draw_windows(np.zeros((0, 4), np.float32), 375, 500, 16, seed=9, step=4, image=2,
                                         return_attempts=True)
    assert (attempts == 1).all() and (wins == wins[0]).all() and wins[0, 2] > wins[0, 0]
    lab = labels.window_labels_exact(np.zeros((0, 4), np.float32), np.zeros((0, 5), np.float32), wins, 5, 375, 500)
    assert (lab[:, 0] == 1).all() and lab[:, 1:].sum() == 0


def test_launcher_lists_the_flag_and_trainer_checks_the_mode():
    r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.train", "--help"], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0 and "--aux_labels" in r.stdout and "generate" in r.stdout, r.stdout + r.stderr
    from mtl_ssl_amd import train
    assert train._flags(["--train_dir=x"]).aux_labels == "record"
    assert train._flags(["--train_dir=x", "--aux_labels=generate"]).aux_labels == "generate"
    from mtl_ssl_amd.trainer import Trainer
    with pytest.raises(ValueError, match="aux_labels"):
        Trainer(None, None, aux_labels="sometimes")


@pytest.mark.parametrize("field,mtl", [("window_boxes", dict(window=True, closeness=False, edgemask=False)),
                                       ("groundtruth_edgemask", dict(window=False, closeness=False, edgemask=True)),
                                       ("groundtruth_closeness", dict(window=False, closeness=True, edgemask=False))])
def test_record_mode_names_the_missing_field(field, mtl):
    from mtl_ssl_amd.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr.aux_labels = "record"
    tr.model = types.SimpleNamespace(_mtl=types.SimpleNamespace(**mtl))
    batch = {"groundtruth_boxes": [np.zeros((1, 4), np.float32)], "groundtruth_classes": [np.zeros((1, 5), np.float32)]}
    with pytest.raises(ValueError) as e:
        tr.provide(batch)
    assert field in str(e.value) and "--aux_labels=generate" in str(e.value)
