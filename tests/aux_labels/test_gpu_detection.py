"""The label kernels of csrc/aux_labels.hip against their host definitions (mtl_ssl_amd/labels.py): window soft labels
on the golden file's own windows and against window_labels_exact on random and degenerate box sets up to the LDS
bound, the window draw bit for bit against draw_windows, closeness and the edge mask against closeness_labels_exact /
edgemask_exact and the golden file, and every kernel twice on the same inputs.

The module shares its name with tests/test_gpu_detection.py on purpose: tests/conftest.py orders the GPU suite by module
name, and these are kernel-level parity tests."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ULP = 2.0 ** -23            # both sides compute in double and round once to float32: one float32 ulp of a value in [0, 1]
HALF_UNIT = 5e-4 + 1e-6     # half a unit of the golden file's third decimal + the float32 normalisation of its pixel boxes


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    return ops


def _gold():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "aux_labels_golden.json")))["cases"]


def _norm(abs_boxes, H, W):
    b = np.asarray(abs_boxes, np.float64).reshape(-1, 4)
    return (b / [H, W, H, W]).astype(np.float32)


def _device_gt(boxes_list, ids_list, K, Gmax=None):
    """What provide_groundtruth leaves on the device; rows past num hold NaN boxes and a stray class (never read)."""
    B = len(boxes_list)
    G = Gmax or max(max(len(b) for b in boxes_list), 1)
    boxes = np.full((B, G, 4), np.nan, np.float32)
    cls = np.zeros((B, G, K + 1), np.float32)
    cls[:, :, K] = 1
    for i, (b, ids) in enumerate(zip(boxes_list, ids_list)):
        n = len(b)
        boxes[i, :n] = b
        cls[i, :n] = 0
        cls[i, np.arange(n), np.asarray(ids, np.int64)] = 1
    dev = torch.device("cuda")
    num = torch.tensor([len(b) for b in boxes_list], dtype=torch.int32, device=dev)
    return torch.from_numpy(boxes).to(dev), torch.from_numpy(cls).to(dev), num


def _random_boxes(rng, G, lo=0.03, hi=0.7):
    cyx, hw = rng.uniform(0, 1, (G, 2)), rng.uniform(lo, hi, (G, 2))
    return np.concatenate([cyx - hw / 2, cyx + hw / 2], 1).clip(0, 1).astype(np.float32)


def _random_windows(rng, n):
    lo, size = rng.uniform(0, 0.6, (n, 2)), rng.uniform(0.1, 0.6, (n, 2))
    w = np.concatenate([lo, np.minimum(lo + size, 1.0)], 1)
    return np.concatenate([w, [[0, 0, 1, 1]]]).astype(np.float32)           # the last window is the image


def test_window_labels_on_the_golden_windows(ops):
    """The reference's own draws and labels: at most 1.5 units of the third decimal anywhere, half a unit on 99.5 % of
    the entries (its inclusion-exclusion and a sweep can land on opposite sides of a rounding boundary)."""
    diffs = []
    for c in _gold():
        K, W, H = c["K"], c["width"], c["height"]
        boxes, ids = _norm(c["boxes"], H, W), c["classes"]
        windows = np.asarray(c["window_boxes"], np.float32)
        b, cl, num = _device_gt([boxes], [ids], K)
        got = ops.aux_window_labels(b, cl, num, torch.from_numpy(windows[None]).cuda(), (H, W)).cpu().numpy()[0]
        assert got.shape == (len(windows), K + 1)
        diffs.append(np.abs(got.astype(np.float64) - np.asarray(c["window_labels"])).ravel())
    d = np.concatenate(diffs)
    print("window labels vs golden: max %.3e, within half a unit %.5f" % (d.max(), (d <= HALF_UNIT).mean()))
    assert d.max() <= 1.5e-3 and (d <= HALF_UNIT).mean() >= 0.995


def _window_cases():
    rng = np.random.RandomState(21)
    cases = []
    for G, K in ((1, 5), (2, 5), (7, 20), (23, 20), (40, 90), (64, 90), (100, 90), (128, 90), (128, 5), (256, 90)):
        boxes = _random_boxes(rng, G)
        cases.append(("random%d" % G, K, boxes, rng.randint(1, K + 1, G)))
    b = _random_boxes(rng, 6)
    cases.append(("duplicates", 5, np.concatenate([b, b, b[:2]]), np.r_[rng.randint(1, 6, 6), rng.randint(1, 6, 6), 1, 1]))
    grid = np.array([[y, x, y + 0.25, x + 0.25] for y in (0, 0.25, 0.5, 0.75) for x in (0, 0.25, 0.5, 0.75)], np.float32)
    cases.append(("shared_edges", 5, grid, np.arange(16) % 3 + 1))
    cases.append(("tiling_one_class", 5, grid, np.ones(16, np.int64)))
    z = _random_boxes(rng, 8)
    z[::2, 2] = z[::2, 0]                                                   # zero height
    z[1, 3] = z[1, 1]                                                       # zero width
    cases.append(("zero_area", 5, z, rng.randint(1, 6, 8)))
    cases.append(("corner_boxes", 20, _random_boxes(rng, 12, 0.02, 0.1) * 0.2, rng.randint(1, 21, 12)))
    cases.append(("one_box_is_the_image", 5, np.array([[0, 0, 1, 1], [0.2, 0.2, 0.4, 0.4]], np.float32), [2, 3]))
    cases.append(("no_boxes", 5, np.zeros((0, 4), np.float32), np.zeros((0,), np.int64)))
    return cases, rng


def test_window_labels_match_the_exact_definition(ops):
    from mtl_ssl_amd import labels
    cases, rng = _window_cases()
    worst = 0.0
    for name, K, boxes, ids in cases:
        H, W = int(rng.randint(200, 700)), int(rng.randint(200, 900))
        windows = _random_windows(rng, 5)
        if name == "corner_boxes":                                          # most windows miss every box
            windows[0] = [0.5, 0.5, 0.9, 0.9]
        Gmax = max(len(boxes), 1) + (3 if len(boxes) not in (128, 256) else 0)
        b, cl, num = _device_gt([boxes], [ids], K, Gmax)
        got = ops.aux_window_labels(b, cl, num, torch.from_numpy(windows[None]).cuda(), (H, W)).cpu().numpy()[0]
        want = labels.window_labels_exact(boxes, ids, windows, K, H, W)
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst = max(worst, err)
        assert err <= ULP, (name, err)
        assert np.isfinite(got).all() and abs(float(got.astype(np.float64).sum(1).max()) - 1) < 1e-5
    print("window labels vs window_labels_exact: max abs err %.3e over %d cases" % (worst, len(cases)))


def test_window_labels_in_a_batch_use_each_image_s_own_boxes(ops):
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(5)
    K, H, W = 20, 600, 800
    bl = [_random_boxes(rng, g) for g in (9, 0, 31, 1)]
    il = [rng.randint(1, K + 1, len(b)) for b in bl]
    wl = np.stack([_random_windows(rng, 7) for _ in bl])
    b, cl, num = _device_gt(bl, il, K)
    got = ops.aux_window_labels(b, cl, num, torch.from_numpy(wl).cuda(), (H, W)).cpu().numpy()
    for i in range(len(bl)):
        want = labels.window_labels_exact(bl[i], il[i], wl[i], K, H, W)
        assert np.abs(got[i].astype(np.float64) - want).max() <= ULP, i


def test_label_kernels_refuse_more_boxes_than_they_hold(ops):
    from mtl_ssl_amd.lib import MtlsslError
    assert ops.AUX_MAX_GT >= 128
    G = ops.AUX_MAX_GT + 1
    rng = np.random.RandomState(0)
    b, cl, num = _device_gt([_random_boxes(rng, G)], [np.ones(G, np.int64)], 5)
    win = torch.tensor([[[0, 0, 1, 1]]], dtype=torch.float32, device="cuda")
    for call in (lambda: ops.aux_window_labels(b, cl, num, win, (300, 400)), lambda: ops.aux_closeness(b, cl, num, (300, 400)),
                 lambda: ops.aux_edgemask(b, num, (300, 400))):
        with pytest.raises(MtlsslError, match="at most %d" % ops.AUX_MAX_GT):
            call()


def test_draw_windows_equal_the_host_function_bit_for_bit(ops):
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(8)
    small = np.array([[0.55, 0.6, 0.8, 0.85]], np.float32)                  # 6 % of the image: windows get redrawn
    pool = [_random_boxes(rng, 5, 0.25, 0.5), np.zeros((0, 4), np.float32), small, _random_boxes(rng, 17, 0.2, 0.5)]
    redraws = 0
    for B in (1, 2, 4):
        for (H, W), Wn in (((600, 800), 64), ((160, 224), 6), ((375, 500), 64)):
            bl = [pool[(i + B) % 4] for i in range(B)]
            b, _, num = _device_gt(bl, [np.ones(len(x), np.int64) for x in bl], 5, 20)
            for seed, step, image0 in ((0, 0, 0), (1, 0, 0), (1, 7, 0), (1, 7, 4), (2 ** 31 + 5, 123456, 30)):
                got = ops.aux_draw_windows(b, num, Wn, (H, W), seed, step, image0).cpu().numpy()
                for i in range(B):
                    want, attempts = labels.draw_windows(bl[i], H, W, Wn, seed, step, image0 + i, return_attempts=True)
                    assert attempts.max() < labels.WINDOW_ATTEMPTS          # nothing passes by the attempt cap
                    redraws += int((attempts > 1).sum())
                    np.testing.assert_array_equal(got[i], want)
                    if not len(bl[i]):
                        assert (got[i] == got[i][0]).all()
    assert redraws > 100


def test_closeness_matches_the_exact_definition(ops):
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(13)
    worst = 0.0
    for K, sizes in ((5, (1, 2, 6, 0)), (20, (23, 3)), (90, (100, 128, 1)), (90, (256,))):
        H, W = int(rng.randint(200, 700)), int(rng.randint(200, 900))
        bl = [_random_boxes(rng, g) for g in sizes]
        il = [rng.randint(1, K + 1, g) for g in sizes]
        b, cl, num = _device_gt(bl, il, K)
        got = ops.aux_closeness(b, cl, num, (H, W)).cpu().numpy()
        assert got.shape == (len(sizes), max(max(sizes), 1), K + 1)
        for i, g in enumerate(sizes):
            assert (got[i, g:] == 0).all()                                  # rows beyond num
            if g:
                want = labels.closeness_labels_exact(bl[i], il[i], K, H, W)
                worst = max(worst, float(np.abs(got[i, :g].astype(np.float64) - want).max()))
                assert np.abs(got[i, :g].astype(np.float64) - want).max() <= ULP, (K, g)
            if g == 1:
                assert got[i, 0, 0] == 1 and (got[i, 0, 1:] == 0).all()
    # objects of one class only: nothing of another class is around
    bl, il = [_random_boxes(rng, 4)], [np.full(4, 3)]
    b, cl, num = _device_gt(bl, il, 5)
    got = ops.aux_closeness(b, cl, num, (300, 400)).cpu().numpy()[0]
    assert (got[:, 0] == 1).all() and (got[:, 1:] == 0).all()
    for c in _gold():
        if len(c["boxes"]):
            K, W, H = c["K"], c["width"], c["height"]
            b, cl, num = _device_gt([_norm(c["boxes"], H, W)], [c["classes"]], K)
            d = np.abs(ops.aux_closeness(b, cl, num, (H, W)).cpu().numpy()[0].astype(np.float64) - np.asarray(c["closeness"]))
            assert d.max() <= 1.5e-3 and (d <= HALF_UNIT).mean() >= 0.995
    print("closeness vs closeness_labels_exact: max abs err %.3e" % worst)


def test_edgemask_matches_the_exact_definition_and_the_golden_file(ops):
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(17)
    for sizes, mask in (((1, 4, 0), 64), ((30, 128), 64), ((256,), 64), ((5, 2), 32), ((3,), 100)):
        H, W = int(rng.randint(200, 700)), int(rng.randint(200, 900))
        bl = [_random_boxes(rng, g, 0.005, 0.6) for g in sizes]
        if sizes[0] == 1:
            bl[0] = np.array([[0.3, 1.0, 0.5, 1.0]], np.float32)            # on the right border: the zero-width fix-up
        b, _, num = _device_gt(bl, [np.ones(g, np.int64) for g in sizes], 5)
        got = ops.aux_edgemask(b, num, (H, W), mask).cpu().numpy()
        assert got.shape == (len(sizes), 2, mask, mask)
        for i in range(len(sizes)):
            want = labels.edgemask_exact(bl[i], H, W, mask)
            np.testing.assert_array_equal(got[i, 0], want[0])
            np.testing.assert_allclose(got[i, 1], want[1], rtol=1e-6, atol=0)
    for c in _gold():
        W, H = c["width"], c["height"]
        boxes = _norm(c["boxes"], H, W)
        b, _, num = _device_gt([boxes], [np.ones(len(boxes), np.int64)], 5)
        em = ops.aux_edgemask(b, num, (H, W)).cpu().numpy()[0]
        np.testing.assert_array_equal(em[0].astype(int), np.asarray(c["edgemask_fg"]))
        np.testing.assert_allclose(em[1].astype(np.float64).sum(1), c["edgemask_weight_sum_rows"], rtol=1e-5)
        np.testing.assert_allclose(em[1].astype(np.float64)[::7, ::5], c["edgemask_weight_probe"], rtol=1e-5)


def test_label_kernels_give_the_same_bits_twice(ops):
    rng = np.random.RandomState(29)
    K, H, W = 90, 600, 800
    bl = [_random_boxes(rng, g) for g in (100, 8)]
    il = [rng.randint(1, K + 1, len(x)) for x in bl]
    b, cl, num = _device_gt(bl, il, K)

    def run():
        wb = ops.aux_draw_windows(b, num, 64, (H, W), 3, 11, 0)
        return wb, ops.aux_window_labels(b, cl, num, wb, (H, W)), ops.aux_closeness(b, cl, num, (H, W)), \
            ops.aux_edgemask(b, num, (H, W))
    first = [t.clone() for t in run()]
    torch.cuda.synchronize()
    for x, y in zip(first, run()):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
