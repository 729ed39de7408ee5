"""mtlssl_coco_match against CocoDetectionEvaluator._evaluate_image, which defines its semantics: every comparison is
np.array_equal (dtm, dig, the groundtruth counts) over all four area ranges, all ten thresholds and maxDets 1 / 10 / 100
— the work is exact, so there is no tolerance anywhere in this module.

Hand-made segments sit on every rule (tests/coco_eval/cases.py: empty sides, an IoU exactly on a threshold, identical
groundtruth, a crowd box claimed again, regular before ignored, areas on the range edges, an unmatched detection out of
range, 100 detections, 70 groundtruth boxes = more than one 64-lane pass of the IoU step, the cap and one box above it,
which the evaluator keeps on the host). A random set then compares evaluate() of a device-backed evaluator with the
host's, number for number.

The module shares its name with tests/test_gpu_detection.py on purpose: tests/conftest.py orders the GPU suite by module
name, and these kernel-level tests run in its first stage, ahead of every whole-model case."""
import numpy as np
import pytest
import torch

from tests.coco_eval import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _evaluator(K, device=None, cap=100):
    from mtl_ssl_amd.evaluation import CocoDetectionEvaluator
    return CocoDetectionEvaluator(K, cap, device=device)


def test_hand_made_segments_equal_the_host_match():
    from mtl_ssl_amd import ops
    ev = cases.fill_hand_made(_evaluator(3, DEV), ops.COCO_MATCH_MAX_GT)
    tab, dtm, dig, npig = ev.match_on_device(cases.keys_of(ev))
    names = [c[0] for c in cases.hand_made(ops.COCO_MATCH_MAX_GT)]
    assert len(tab["seg_cat"]) == len(names)
    n_gt = np.diff(tab["gt_off"])
    # the sizes the cases are there for really reach the kernel (and the host path, for the one above the cap)
    assert n_gt.max() == ops.COCO_MATCH_MAX_GT + 1 and ops.COCO_MATCH_MAX_GT in n_gt and 70 in n_gt
    assert np.diff(tab["dt_off"]).max() == 100
    cells = cases.assert_match_equals_host(ev, tab, dtm, dig, npig)
    assert cells == len(names) * 4 * 3
    # the cases do what their names say (host side, so that a change of the inputs cannot hollow them out)
    image = {n: i for i, n in enumerate(names)}            # fill_hand_made: image key i holds case i in category i % K
    host = lambda name: ev._evaluate_image(image[name], image[name] % ev.K, ev.AREA_RNG[0], 100)
    _, m, g, n = host("iou exactly 0.5")
    assert m[:, 0].tolist() == [True] + [False] * 9
    _, m, g, n = host("crowd claimed three times")
    assert m[0].tolist() == [True, True, True, False] and g[0].tolist() == [True, True, True, False] and n == 0
    _, m, g, n = host("regular beats ignored")
    assert m[0].tolist() == [True, True] and g[0].tolist() == [False, True] and g[9].tolist() == [True, True]


def test_detections_beyond_100_per_image_and_the_three_max_dets():
    """max_detections_per_image above the largest maxDets: one run still covers the three slices."""
    ev = cases.fill_random(_evaluator(2, DEV, cap=150), 6, seed=5, max_gt=20, max_dt=150)
    tab, dtm, dig, npig = ev.match_on_device(cases.keys_of(ev))
    assert cases.assert_match_equals_host(ev, tab, dtm, dig, npig) > 0


@pytest.fixture(scope="module")
def random_pair():
    host = cases.fill_random(_evaluator(6), 300, seed=7)
    dev = cases.fill_random(_evaluator(6, DEV), 300, seed=7)
    return host.evaluate(), dev


def test_random_set_evaluates_to_the_hosts_numbers(random_pair):
    want, dev = random_pair
    got = dev.evaluate()
    for k in ("stats", "per_class_ap", "per_class_stats"):
        assert not np.isnan(want[k]).any() and not np.isnan(got[k]).any(), k
        assert want[k].shape == got[k].shape and (want[k] == got[k]).all(), (k, want[k], got[k])
    assert got["per_class_stats"].shape == (6, 12) and (got["per_class_stats"][:, 0] == got["per_class_ap"]).all()
    for name in dev.NAMES:
        assert got[name] == want[name], name
    assert (want["stats"] > 0).sum() >= 10, want["stats"]            # the set exercises the metrics, not only -1 / 0
    assert set(dev.timings) == {"table_build_s", "kernel_s", "copy_s", "accumulate_s"}


def test_two_device_runs_agree(random_pair):
    _, dev = random_pair
    keys = cases.keys_of(dev)
    (_, m1, i1, n1), (_, m2, i2, n2) = dev.match_on_device(keys), dev.match_on_device(keys)
    assert m1.any() and i1.any() and n1.any()
    assert (m1 == m2).all() and (i1 == i2).all() and (n1 == n2).all()


def test_too_many_threshold_range_pairs_is_a_clean_error():
    from mtl_ssl_amd import ops
    from mtl_ssl_amd.lib import MtlsslError
    dev = torch.device(DEV)
    f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    boxes = f64([[0, 0, 10, 10]])
    args = ([0, 1], [0, 1], boxes, boxes, f64([100.0]), torch.zeros(1, dtype=torch.uint8, device=dev))
    rng = f64([[0.0, 1e10]] * 4)
    with pytest.raises(MtlsslError, match="coco_match: 17 IoU thresholds x 4 area ranges"):
        ops.coco_match(*args, f64(np.linspace(0.1, 0.9, 17)), rng)
    with pytest.raises(MtlsslError, match="coco_match: a category of one image has 257 groundtruth boxes"):
        many = f64(np.tile([[0, 0, 10, 10]], (257, 1)))
        ops.coco_match([0, 1], [0, 257], boxes, many, f64(np.full(257, 100.0)),
                       torch.zeros(257, dtype=torch.uint8, device=dev), f64(np.linspace(0.5, 0.95, 10)), rng)
    m, i, n, _ = ops.coco_match(*args, f64(np.linspace(0.1, 0.85, 16)), rng)      # 64 pairs: the largest that fit
    assert m.cpu().numpy().view(np.uint64)[0] == np.uint64(2 ** 64 - 1) and int(i.cpu()[0]) == 0
    assert n.cpu().tolist() == [[1, 1, 1, 1]]
