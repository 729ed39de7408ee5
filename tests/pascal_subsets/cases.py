"""Inputs of the groundtruth-subset tests and the comparisons against the host definition: a subset's result is what
PascalDetectionEvaluator gives for the same images with is_difficult = ~member(subset), and a detection's labels in
mtlssl_pascal_match are what PascalDetectionEvaluator._tp_fp returns for that subset. Everything here is exact work,
so every comparison is np.array_equal / ==."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "pascal_subset_golden.npz")


# ------------------------------------------------------------------------------ the golden set
def golden():
    """-> (images = [(gt boxes, gt classes, difficult, subset strings, dt boxes, dt scores, dt classes)], the file)."""
    z = np.load(GOLDEN)
    images = []
    for i in range(int(z["num_images"])):
        g, d = z["gt_image"] == i, z["dt_image"] == i
        images.append((z["gt_boxes"][g], z["gt_classes"][g], z["gt_difficult"][g], [str(s) for s in z["gt_subset"][g]],
                       z["dt_boxes"][d], z["dt_scores"][d], z["dt_classes"][d]))
    return images, z


def fill(ev, images):
    for i, (gb, gc, gd, gs, db, ds, dc) in enumerate(images):
        ev.add_single_ground_truth_image_info(i, gb, gc, is_difficult=gd, subsets=gs)
        ev.add_single_detected_image_info(i, db, ds, dc)
    return ev


def member(strings, difficult, name):
    return np.asarray([name in s.split("|") for s in strings], bool).reshape(-1) & ~np.asarray(difficult, bool)


def one_run_per_subset(images, names, K, thr=0.5, cap=10000):
    """{name: PascalDetectionEvaluator.evaluate()} with is_difficult = ~member(name): the definition."""
    from mtl_ssl_amd.evaluation import PascalDetectionEvaluator
    out = {}
    for name in names:
        ev = PascalDetectionEvaluator(K, thr, cap)
        for i, (gb, gc, gd, gs, db, ds, dc) in enumerate(images):
            ev.add_single_ground_truth_image_info(i, gb, gc, is_difficult=~member(gs, gd, name))
            ev.add_single_detected_image_info(i, db, ds, dc)
        out[name] = (ev.evaluate(), ev.num_gt.copy())
    return out


def assert_results_equal(got, want):
    """Two PascalSubsetEvaluator.evaluate() results, number for number."""
    assert got["subset_names"] == want["subset_names"]
    for n in want["subset_names"]:
        assert np.array_equal(got["ap_per_class"][n], want["ap_per_class"][n], equal_nan=True), n
        assert got["mean_ap"][n] == want["mean_ap"][n] or (np.isnan(got["mean_ap"][n]) and np.isnan(want["mean_ap"][n]))
        assert np.array_equal(got["num_gt"][n], want["num_gt"][n]), n
        for k in ("precisions", "recalls"):
            assert len(got[k][n]) == len(want[k][n])
            for a, b in zip(got[k][n], want[k][n]):
                assert np.array_equal(a, b), (n, k)
    assert np.array_equal(got["corloc_per_class"], want["corloc_per_class"], equal_nan=True)
    assert got["mean_corloc"] == want["mean_corloc"] or (np.isnan(got["mean_corloc"]) and np.isnan(want["mean_corloc"]))


# ------------------------------------------------------------------------------ hand-made segments
def _grid(n, rng):
    """n distinct groundtruth boxes on a 16-column grid of 10 x 10 cells, each 8 x 8."""
    r, c = np.divmod(np.arange(n), 16)
    return np.stack([10.0 * r, 10.0 * c, 10.0 * r + 8, 10.0 * c + 8], 1)


def _around(gt, n, rng):
    """n detections: jittered copies of random groundtruth boxes (IoUs on both sides of 0.5), distinct scores."""
    b = gt[rng.randint(0, len(gt), n)] + rng.normal(0, 1.0, (n, 4)) * rng.choice([0.6, 2.0], (n, 1))
    return b, rng.permutation(n) / float(n) + 0.001


def _tags(n, S, rng):
    """Subset strings for n boxes over the names s00..s<S-1>: every name is used, one box in eight has none."""
    names = ["s%02d" % j for j in range(S)]
    on = rng.rand(n, S) < 0.5
    on[rng.rand(n) < 0.125] = False
    on[0] = True                                            # the first box names every subset: the union is complete
    return ["|".join(nm for nm, o in zip(names, row) if o) for row in on]


def hand_made(max_gt):
    """[(name, cap, gt boxes [G,4], subset strings [G], dt boxes [D,4], dt scores [D])], one segment each."""
    rng = np.random.RandomState(11)
    f = lambda rows: np.asarray(rows, np.float64).reshape(-1, 4)
    far = [100, 100, 110, 110]                              # a box nobody overlaps; it carries the names a case needs
    out = [
        ("no groundtruth", 10000, f([]), [], f([[0, 0, 2, 2], [1, 1, 3, 3]]), [0.9, 0.8]),
        ("iou exactly 0.5", 10000, f([[0, 0, 2, 2]]), ["a"], f([[0, 0, 2, 1]]), [0.9]),
        ("equal iou first wins", 10000, f([[0, 0, 4, 3], [0, 1, 4, 4]]), ["a", "b"], f([[0, 0, 4, 4]]), [0.9]),
        ("identical groundtruth", 10000, f([[0, 0, 4, 4], [0, 0, 4, 4]]), ["a", "a"],
         f([[0, 0, 4, 4], [0, 0, 4, 4]]), [0.9, 0.8]),
        ("box in a only", 10000, f([[0, 0, 4, 4], far]), ["a", "a|b"], f([[0, 0, 4, 4], [0, 0, 4, 3.5]]), [0.9, 0.8]),
        ("best outside second inside", 10000, f([[0, 0, 10, 10], [0, 0, 10, 6], far]), ["a", "a|b", "b"],
         f([[0, 0, 10, 9]]), [0.9]),
        ("nan groundtruth", 10000, f([[np.nan, 0, 2, 2], [0, 0, 2, 2]]), ["a", "a"], f([[0, 0, 2, 2]]), [0.9]),
        ("zero-area groundtruth", 10000, f([[1, 1, 1, 1], [0, 0, 2, 2]]), ["a", "a"],
         f([[0, 0, 2, 2], [0.5, 0.5, 1.5, 1.5]]), [0.9, 0.8]),
    ]
    g = _grid(6, rng)
    out.append(("cap 5 of 9", 5, g, _tags(6, 3, rng)) + _around(g, 9, rng))
    out.append(("120 detections", 10000, g, _tags(6, 3, rng)) + _around(g, 120, rng))
    for n in (70, max_gt, max_gt + 1):
        g = _grid(n, rng)
        out.append(("%d groundtruth" % n, 10000, g, _tags(n, 3, rng)) + _around(g, 40, rng))
    g = _grid(9, rng)
    for S in (1, 3, 64, 65):
        out.append(("S = %d" % S, 10000, g, _tags(9, S, rng)) + _around(g, 30, rng))
    return out


def case_evaluator(case, device=None, thr=0.5):
    """A one-image, one-class PascalSubsetEvaluator holding the case."""
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    name, cap, gb, gs, db, ds = case
    ev = PascalSubsetEvaluator(1, thr, cap, device=device)
    ev.add_single_ground_truth_image_info(name, gb, np.zeros(len(gb), int), subsets=gs)
    ev.add_single_detected_image_info(name, db, ds, np.zeros(len(db), int))
    if not len(gb):                          # subset names must come from somewhere: an image with a box, no detections
        ev.add_single_ground_truth_image_info("names", [[100, 100, 110, 110]], [0], subsets=["a|b"])
    return ev


def host_labels(ev, case, subset):
    """(scores, tp/fp labels) of _tp_fp for the case in one subset."""
    name, cap, gb, gs, db, ds = case
    return ev._pascal._tp_fp(np.asarray(db, float), np.asarray(ds, float), gb, ~member(gs, np.zeros(len(gs), bool), subset))


def assert_match_equals_host(ev, tab, tp, drop, hit):
    """tp / drop / hit of match_on_device against _tp_fp per subset and iou_matrix(...).max() >= thr, segment by
    segment. With distinct scores, the scores _tp_fp keeps pin `drop` and its labels pin `tp`. Returns the number of
    (segment, subset) pairs compared."""
    from mtl_ssl_amd.evaluation import iou_matrix
    names = ev.subset_names()
    members = ev._members(names)
    assert not (tp & drop).any()
    compared = 0
    for i, (key, c) in enumerate(zip(tab["seg_key"], tab["seg_cat"])):
        d0, d1 = tab["dt_off"][i], tab["dt_off"][i + 1]
        boxes, scores, cls = ev.dt[key]
        db, ds = boxes[cls == c], scores[cls == c]
        assert len(np.unique(ds)) == len(ds)
        gb, gc = ev.gt[key][:2] if key in ev.gt else (np.zeros((0, 4)), np.zeros(0, int))
        mem = members[key][gc == c] if key in members else np.zeros((0, len(names)), bool)
        for s in range(len(names)):
            sc, lab = ev._pascal._tp_fp(db, ds, gb[gc == c], ~mem[:, s])
            keep = ~drop[s, d0:d1]
            assert np.array_equal(sc, tab["dt_scores"][d0:d1][keep]), (key, c, names[s])
            assert np.array_equal(lab, tp[s, d0:d1][keep]), (key, c, names[s])
            compared += 1
        rows = tab["dt_boxes"][d0:d1]
        with np.errstate(invalid="ignore"):
            want = (iou_matrix(rows, gb[gc == c]).max(1) >= ev.thr) if np.any(gc == c) else np.zeros(len(rows), bool)
        assert np.array_equal(hit[d0:d1], want), (key, c)
    return compared


# ------------------------------------------------------------------------------ a random set
def random_images(n_images, K, S, seed, difficult=0.2):
    rng = np.random.RandomState(seed)
    names = ["s%d" % j for j in range(S)]
    images = []
    total = 0
    for i in range(n_images):
        g = int(rng.randint(0, 7))
        c = rng.uniform(0.2, 0.8, (g, 2))
        hw = rng.uniform(0.08, 0.5, (g, 2))
        gb = np.concatenate([c - hw / 2, c + hw / 2], 1)
        gc = rng.randint(0, K, g)
        on = rng.rand(g, S) < 0.6
        gs = ["|".join(nm for nm, o in zip(names, row) if o) for row in on]
        n = int(rng.randint(0, 30))
        db = np.concatenate([rng.uniform(0.2, 0.8, (n, 2))] * 2, 1) + np.concatenate(
            [-rng.uniform(0.04, 0.25, (n, 2)), rng.uniform(0.04, 0.25, (n, 2))], 1)
        dc = rng.randint(0, K, n)
        if g and n:
            near = rng.rand(n) < 0.7
            src = rng.randint(0, g, n)
            db[near] = gb[src[near]] + rng.normal(0, 0.03, (int(near.sum()), 4))
            dc[near] = gc[src[near]]
        images.append([gb, gc, rng.rand(g) < difficult, gs, db, None, dc])
        total += n
    scores = (rng.permutation(total) + 1.0) / (total + 1.0)                  # all distinct
    off = 0
    for im in images:
        im[5] = scores[off:off + len(im[4])]
        off += len(im[4])
    return [tuple(im) for im in images]
