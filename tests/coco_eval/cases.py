"""Shared inputs of the COCO-evaluator tests: hand-made (image, category) segments, a random evaluator filling, the
comparison of a match table against CocoDetectionEvaluator._evaluate_image, and a numpy restatement of the lane rule of
mtlssl_coco_match (one (threshold, area range) pair walks the detections in order with its own claimed set; regular
boxes in input order, then ignored ones)."""
import numpy as np

from mtl_ssl_amd.evaluation import CocoDetectionEvaluator


def _boxes(rows):
    return np.asarray(rows, np.float64).reshape(-1, 4)


def hand_made(max_gt):
    """[(name, gt boxes, crowd, areas or None, dt boxes, scores)]: one image, one category each."""
    rng = np.random.RandomState(3)

    def rand_boxes(n, size=200.0, smallest=4.0):
        yx = rng.uniform(0, size, (n, 2))
        hw = rng.uniform(smallest, 120, (n, 2))
        return np.concatenate([yx, yx + hw], 1)

    def jitter(b, amount=6.0):
        return b + rng.uniform(-amount, amount, b.shape)

    cases = []
    cases.append(("no detection", _boxes([[0, 0, 50, 50]]), [0], None, _boxes([]), []))
    cases.append(("no groundtruth", _boxes([]), [], None, _boxes([[0, 0, 50, 50], [0, 0, 10, 10]]), [0.9, 0.8]))
    cases.append(("iou exactly 0.5", _boxes([[0, 0, 10, 20]]), [0], None, _boxes([[0, 0, 10, 10]]), [0.9]))
    cases.append(("identical groundtruth", _boxes([[10, 10, 60, 60]] * 2), [0, 0], None,
                  _boxes([[10, 10, 60, 60], [10, 10, 60, 60], [10, 10, 60, 61]]), [0.9, 0.8, 0.7]))
    cases.append(("identical ignored groundtruth", _boxes([[10, 10, 60, 60]] * 2), [0, 1], [1e6, 2500.0],
                  _boxes([[10, 10, 60, 60]] * 3), [0.9, 0.8, 0.7]))
    cases.append(("crowd claimed three times", _boxes([[0, 0, 100, 100]]), [1], None,
                  _boxes([[0, 0, 40, 40], [50, 50, 90, 90], [10, 10, 30, 80], [300, 300, 340, 340]]),
                  [0.9, 0.8, 0.7, 0.6]))
    # the crowd box has the higher IoU (intersection over detection area = 1), the regular box still wins
    cases.append(("regular beats ignored", _boxes([[0, 0, 100, 100], [10, 10, 50, 50]]), [1, 0], None,
                  _boxes([[10, 10, 50, 56], [12, 12, 50, 50]]), [0.9, 0.8]))
    cases.append(("areas on the range edges", _boxes([[0, 0, 32, 32], [100, 100, 196, 196]]), [0, 0], None,
                  _boxes([[0, 0, 32, 32], [100, 100, 196, 196], [0, 0, 31, 33]]), [0.9, 0.8, 0.7]))
    cases.append(("unmatched detection out of range", _boxes([[0, 0, 40, 40]]), [0], None,
                  _boxes([[200, 200, 210, 210], [200, 200, 400, 400], [0, 0, 40, 41]]), [0.9, 0.8, 0.7]))
    g = rand_boxes(5, smallest=40.0)                       # no jittered copy turns inside out: all 100 are valid
    cases.append(("100 detections", g, [0, 0, 1, 0, 0], None, jitter(g[rng.randint(0, 5, 100)], 12.0),
                  np.round(rng.uniform(0, 1, 100), 2)))
    g = rand_boxes(70)
    cases.append(("70 groundtruth", g, rng.uniform(size=70) < 0.25, None, jitter(g[rng.randint(0, 70, 40)]),
                  np.round(rng.uniform(0, 1, 40), 2)))
    g = rand_boxes(max_gt)
    cases.append(("groundtruth at the cap", g, rng.uniform(size=max_gt) < 0.25, None,
                  jitter(g[rng.randint(0, max_gt, 30)]), np.round(rng.uniform(0, 1, 30), 2)))
    g = rand_boxes(max_gt + 1)
    cases.append(("groundtruth above the cap", g, rng.uniform(size=max_gt + 1) < 0.25, None,
                  jitter(g[rng.randint(0, max_gt + 1, 30)]), np.round(rng.uniform(0, 1, 30), 2)))
    return cases


def fill_hand_made(ev, max_gt):
    """Every hand-made segment as an image of its own (category = image index modulo ev.K)."""
    for i, (_, gb, crowd, areas, db, ds) in enumerate(hand_made(max_gt)):
        k = i % ev.K
        ev.add_single_ground_truth_image_info(i, gb, np.full(len(gb), k), np.asarray(crowd, bool), areas)
        ev.add_single_detected_image_info(i, db, ds, np.full(len(db), k))
    return ev


def fill_random(ev, num_images, seed, max_gt=6, max_dt=12):
    """Random images over ev.K categories: scores rounded to one decimal (ties across and inside images), a quarter of
    the groundtruth crowd, detections that are jittered groundtruth boxes or noise, areas across the three ranges."""
    rng = np.random.RandomState(seed)
    for i in range(num_images):
        G, D = rng.randint(0, max_gt + 1), rng.randint(0, max_dt + 1)
        yx = rng.uniform(0, 300, (G, 2))
        hw = rng.uniform(8, 160, (G, 2))
        gb = np.concatenate([yx, yx + hw], 1)
        gc = rng.randint(0, ev.K, G)
        ev.add_single_ground_truth_image_info(i, gb, gc, rng.uniform(size=G) < 0.25)
        if G:
            src = rng.randint(0, G, D)
            db = gb[src] + rng.uniform(-10, 10, (D, 4))
            dc = np.where(rng.uniform(size=D) < 0.8, gc[src], rng.randint(0, ev.K, D))
        else:
            yx = rng.uniform(0, 300, (D, 2))
            db = np.concatenate([yx, yx + rng.uniform(8, 160, (D, 2))], 1)
            dc = rng.randint(0, ev.K, D)
        ev.add_single_detected_image_info(i, db, np.round(rng.uniform(0, 1, D), 1), dc)
    return ev


def keys_of(ev):
    return sorted(set(ev.gt) | set(ev.dt), key=str)


def assert_match_equals_host(ev, tab, dtm, dig, npig):
    """dtm / dig [T,A,ND] and npig [S,A] of the segment tables against _evaluate_image: every segment, all four area
    ranges, all ten thresholds, maxDets 1 / 10 / 100. Returns how many (segment, range, maxDets) cells were compared."""
    keys, cells = keys_of(ev), 0
    assert dtm.shape == dig.shape == (len(ev.IOU_THRS), len(ev.AREA_RNG), len(tab["dt_boxes"]))
    for s in range(len(tab["seg_cat"])):
        key, k = keys[tab["seg_img"][s]], int(tab["seg_cat"][s])
        d0 = tab["dt_off"][s]
        for a, rng in enumerate(ev.AREA_RNG):
            for md in ev.MAX_DETS:
                scores, want_m, want_i, want_n = ev._evaluate_image(key, k, rng, md)
                n = len(scores)
                assert n == min(md, tab["dt_off"][s + 1] - d0)
                assert np.array_equal(tab["dt_scores"][d0:d0 + n], scores), (key, k)
                assert np.array_equal(dtm[:, a, d0:d0 + n], want_m), ("dtm", key, k, a, md)
                assert np.array_equal(dig[:, a, d0:d0 + n], want_i), ("dig", key, k, a, md)
                assert int(npig[s, a]) == want_n, ("npig", key, k, a)
                cells += 1
    return cells


def simulate_lanes(tab, iou_thrs, area_rng):
    """The kernel's rule in numpy, from the same segment tables: -> dtm, dig [T,A,ND] bool, npig [S,A]."""
    T, A, ND, S = len(iou_thrs), len(area_rng), len(tab["dt_boxes"]), len(tab["seg_cat"])
    dtm, dig = np.zeros((T, A, ND), bool), np.zeros((T, A, ND), bool)
    npig = np.zeros((S, A), np.int64)
    for s in range(S):
        d0, d1, g0, g1 = tab["dt_off"][s], tab["dt_off"][s + 1], tab["gt_off"][s], tab["gt_off"][s + 1]
        db, gb = tab["dt_boxes"][d0:d1], tab["gt_boxes"][g0:g1]
        crowd, garea = tab["gt_crowd"][g0:g1].astype(bool), tab["gt_area"][g0:g1]
        G = g1 - g0
        ious = CocoDetectionEvaluator._iou(db, gb, crowd) if len(db) and G else np.zeros((len(db), G))
        darea = (db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1])
        for a, (lo, hi) in enumerate(area_rng):
            ignored = crowd | (garea < lo) | (garea > hi)
            npig[s, a] = int(np.sum(~ignored))
            for t, thr in enumerate(iou_thrs):
                claimed = np.zeros(G, bool)
                for di in range(len(db)):
                    best, m = min(thr, 1 - 1e-10), -1
                    for g in range(G):
                        if ignored[g] or claimed[g] or ious[di, g] < best:
                            continue
                        best, m = ious[di, g], g
                    if m < 0:
                        for g in range(G):
                            if not ignored[g] or (claimed[g] and not crowd[g]) or ious[di, g] < best:
                                continue
                            best, m = ious[di, g], g
                    if m >= 0:
                        dtm[t, a, d0 + di], dig[t, a, d0 + di], claimed[m] = True, ignored[m], True
                    else:
                        dig[t, a, d0 + di] = darea[di] < lo or darea[di] > hi
    return dtm, dig, npig
