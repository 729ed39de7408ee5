"""mtlssl_pascal_match against PascalDetectionEvaluator._tp_fp, which defines its semantics: every comparison is
np.array_equal of tp / drop / hit against _tp_fp run once per subset and iou_matrix(...).max() >= thr — the work is
exact, so there is no tolerance anywhere in this module.

Hand-made segments sit on every rule (tests/pascal_subsets/cases.py: no groundtruth, an IoU exactly on the threshold,
equal IoUs, identical boxes, a box in one subset only, the best box outside the subset, a NaN and a zero-area box, the
cap, 120 detections, 70 groundtruth boxes = more than one 64-lane pass, the limit and one box above it, which the
evaluator keeps on the host, 1 / 3 / 64 subsets and 65, which take the host path). A random set then compares
evaluate() of a device-backed evaluator with the host's, number for number.

The module shares its name with tests/test_gpu_detection.py on purpose: tests/conftest.py orders the GPU suite by module
name, and these kernel-level tests run in its first stage, ahead of every whole-model case."""
import numpy as np
import pytest
import torch

from tests.pascal_subsets import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_GT = 256


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert ops.PASCAL_MATCH_MAX_GT == MAX_GT and ops.PASCAL_MATCH_MAX_SUBSETS == 64


HAND_MADE = cases.hand_made(MAX_GT)
ON_DEVICE = [c for c in HAND_MADE if c[0] != "S = 65"]


def _match(case):
    ev = cases.case_evaluator(case, DEV)
    names = ev.subset_names()
    tab, tp, drop, hit = ev.match_on_device(ev._members(names), len(names))
    return ev, names, tab, tp, drop, hit


@pytest.mark.parametrize("case", ON_DEVICE, ids=[c[0] for c in ON_DEVICE])
def test_hand_made_segment_equals_the_host_labelling(case):
    ev, names, tab, tp, drop, hit = _match(case)
    assert len(tab["seg_key"]) == 1 and tp.shape == drop.shape == (len(names), len(hit))
    assert cases.assert_match_equals_host(ev, tab, tp, drop, hit) == len(names)
    # the sizes the cases are there for really reach the kernel (and the host loop, for the one above the limit)
    name, cap, gb, gs, db, ds = case
    valid = int(((db[:, 0] < db[:, 2]) & (db[:, 1] < db[:, 3])).sum())           # _remove_invalid_boxes
    assert np.diff(tab["gt_off"]).tolist() == [len(gb)] and len(hit) == min(valid, cap) >= min(len(db), cap) - 1
    sizes = {"70 groundtruth": (70, 40), "%d groundtruth" % MAX_GT: (MAX_GT, 40),
             "%d groundtruth" % (MAX_GT + 1): (MAX_GT + 1, 40), "cap 5 of 9": (6, 5), "120 detections": (6, 120)}
    if name in sizes:
        assert (len(gb), len(hit)) == sizes[name]
    if name.startswith("S = "):
        assert len(names) == int(name[4:])
    if len(gb) > 6:
        assert tp.any() and drop.any() and hit.any() and not hit.all()


def test_the_cases_do_what_their_names_say():
    """Host side, so that a change of the inputs cannot hollow the cases out."""
    case = {c[0]: c for c in HAND_MADE}
    assert [c[0] for c in HAND_MADE] == [
        "no groundtruth", "iou exactly 0.5", "equal iou first wins", "identical groundtruth", "box in a only",
        "best outside second inside", "nan groundtruth", "zero-area groundtruth", "cap 5 of 9", "120 detections",
        "70 groundtruth", "256 groundtruth", "257 groundtruth", "S = 1", "S = 3", "S = 64", "S = 65"]
    host = lambda name, subset: [x.tolist() for x in cases.host_labels(cases.case_evaluator(case[name]), case[name], subset)]
    assert host("no groundtruth", "a") == [[0.9, 0.8], [False, False]]
    assert host("iou exactly 0.5", "a") == [[0.9], [True]]
    assert host("equal iou first wins", "a") == [[0.9], [True]] and host("equal iou first wins", "b") == [[], []]
    assert host("identical groundtruth", "a") == [[0.9, 0.8], [True, False]]         # the second box is never reached
    assert host("box in a only", "a") == [[0.9, 0.8], [True, False]] and host("box in a only", "b") == [[], []]
    assert host("best outside second inside", "a") == [[0.9], [True]]
    assert host("best outside second inside", "b") == [[], []]                        # dropped, not re-matched
    assert host("nan groundtruth", "a") == [[0.9], [False]]                           # arg-max lands on the NaN box
    assert host("zero-area groundtruth", "a") == [[0.9, 0.8], [True, False]]
    assert len(host("cap 5 of 9", "s00")[0]) <= 5 and len(case["cap 5 of 9"][4]) == 9
    for S in (1, 3, 64, 65):
        assert len(cases.case_evaluator(case["S = %d" % S]).subset_names()) == S


def test_more_than_64_subsets_take_the_host_path_and_agree():
    case = {c[0]: c for c in HAND_MADE}["S = 65"]
    host, dev = cases.case_evaluator(case).evaluate(), cases.case_evaluator(case, DEV)
    got = dev.evaluate()
    assert "match_s" in dev.timings and "kernel_s" not in dev.timings
    assert len(got["subset_names"]) == 65
    cases.assert_results_equal(got, host)


@pytest.fixture(scope="module")
def random_pair():
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    images = cases.random_images(300, 6, 4, seed=7)
    host = cases.fill(PascalSubsetEvaluator(6), images)
    dev = cases.fill(PascalSubsetEvaluator(6, device=DEV), images)
    return host.evaluate(), dev


def test_random_set_evaluates_to_the_hosts_numbers(random_pair):
    want, dev = random_pair
    got = dev.evaluate()
    assert set(dev.timings) == {"table_build_s", "kernel_s", "copy_s", "accumulate_s"}
    assert len(got["subset_names"]) == 4
    cases.assert_results_equal(got, want)
    aps = np.stack([want["ap_per_class"][n] for n in want["subset_names"]])
    assert (aps > 0).sum() >= 20 and not np.isnan(aps).any(), aps                     # not vacuous
    assert len({want["mean_ap"][n] for n in want["subset_names"]}) == 4               # the subsets really differ


def test_random_set_labels_equal_the_host_labelling(random_pair):
    _, dev = random_pair
    names = dev.subset_names()
    tab, tp, drop, hit = dev.match_on_device(dev._members(names), len(names))
    assert cases.assert_match_equals_host(dev, tab, tp, drop, hit) == 4 * len(tab["seg_key"]) > 1000


def test_two_device_runs_agree(random_pair):
    _, dev = random_pair
    names = dev.subset_names()
    members = dev._members(names)
    (_, t1, d1, h1), (_, t2, d2, h2) = dev.match_on_device(members, 4), dev.match_on_device(members, 4)
    assert t1.any() and d1.any() and h1.any()
    assert (t1 == t2).all() and (d1 == d2).all() and (h1 == h2).all()


def test_limits_are_clean_errors():
    from mtl_ssl_amd import ops
    from mtl_ssl_amd.lib import MtlsslError
    dev = torch.device(DEV)
    f64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    boxes = f64([[0, 0, 10, 10]])
    one = torch.ones(1, dtype=torch.int64, device=dev)
    with pytest.raises(MtlsslError, match="pascal_match: 65 subsets"):
        ops.pascal_match([0, 1], [0, 1], boxes, boxes, one, 0.5, 65)
    with pytest.raises(MtlsslError, match="pascal_match: a class of one image has 257 groundtruth boxes"):
        ops.pascal_match([0, 1], [0, 257], boxes, f64(np.tile([[0, 0, 10, 10]], (257, 1))),
                         torch.ones(257, dtype=torch.int64, device=dev), 0.5, 1)
    tp, drop, hit, _ = ops.pascal_match([0, 1], [0, 1], boxes, boxes, -one, 0.5, 64)      # 64 subsets: all that fit
    assert tp.cpu().numpy().view(np.uint64)[0] == np.uint64(2 ** 64 - 1) and int(drop.cpu()[0]) == 0
    assert hit.cpu().tolist() == [1]
