#!/usr/bin/env python3
"""Generate tests/golden/pascal_subset_golden.npz: the reference's ObjectDetectionEvaluation(subset_names=...) on a
seeded detection set with groundtruth subsets.

Run in the authoring container only (needs /root/reference):
    python tests/golden/make_subset_golden.py

The reference class (utils/object_detection_evaluation.py:42-286) is fed as eval_util.py:336-359 feeds it: per image
the subset strings with '' in place of a difficult box's, then the detections. pycocotools, which the module imports
for its COCO class only, is stubbed. 40 images, 3 classes, three overlapping subsets by box area (small < 0.06,
mid in [0.03, 0.2), large >= 0.12), one box in eight in no subset at all, 20 % of the boxes difficult, image 3 without
groundtruth, image 5 without detections, all scores distinct (the reference's argsort is not stable). Stored, data only:
  gt_boxes [NG,4] float64, gt_classes [NG] int64, gt_difficult [NG] bool, gt_subset [NG] str, gt_image [NG] int64
  dt_boxes [ND,4] float64, dt_scores [ND] float64, dt_classes [ND] int64, dt_image [ND] int64
  num_images, num_classes, iou_threshold
  subset_names [S] str (sorted), ap [S,K], mean_ap [S], num_gt [S,K], corloc [K], mean_corloc
"""
import builtins
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
N_IMG, K, THR = 40, 3, 0.5
RANGES = (("small", 0.0, 0.06), ("mid", 0.03, 0.2), ("large", 0.12, np.inf))


def make_set(rng):
    gt, dt = [], []
    for i in range(N_IMG):
        g = 0 if i == 3 else int(rng.randint(1, 6))
        c = rng.uniform(0.2, 0.8, (g, 2))
        hw = rng.uniform(0.08, 0.6, (g, 2))
        gb = np.clip(np.concatenate([c - hw / 2, c + hw / 2], 1), 0.0, 1.0)
        gc = rng.randint(0, K, g)
        area = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
        names = ["|".join(n for n, lo, hi in RANGES if lo <= a < hi) for a in area]
        names = ["" if rng.rand() < 0.125 else n for n in names]
        gt.append((gb, gc, rng.rand(g) < 0.2, names))
        n = 0 if i == 5 else int(rng.randint(4, 25))
        # detections: jittered copies of the groundtruth boxes (so that IoUs straddle the threshold) and random boxes
        src = rng.randint(0, max(g, 1), n)
        near = rng.rand(n) < (0.7 if g else 0.0)
        rc = rng.uniform(0.2, 0.8, (n, 2))
        rhw = rng.uniform(0.08, 0.6, (n, 2))
        db = np.concatenate([rc - rhw / 2, rc + rhw / 2], 1)
        dc = rng.randint(0, K, n)
        if g:
            db[near] = gb[src[near]] + rng.normal(0, 0.04, (int(near.sum()), 4))
            dc[near] = np.where(rng.rand(int(near.sum())) < 0.85, gc[src[near]], dc[near])
        db = np.clip(db, 0.0, 1.0)
        ok = (db[:, 0] < db[:, 2]) & (db[:, 1] < db[:, 3])
        dt.append((db[ok], dc[ok]))
    total = sum(len(d[0]) for d in dt)
    while True:
        scores = rng.uniform(0.01, 1.0, total)
        if len(np.unique(scores)) == total:
            break
    out, off = [], 0
    for db, dc in dt:
        out.append((db, scores[off:off + len(db)], dc))
        off += len(db)
    return gt, out


def main():
    builtins.xrange = range
    for alias, t in (("bool", bool), ("float", float), ("int", int)):      # numpy aliases the 2018 sources still use
        if not hasattr(np, alias):
            setattr(np, alias, t)
    for name in ("pycocotools", "pycocotools.coco", "pycocotools.cocoeval"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pycocotools.coco"].COCO = object
    sys.modules["pycocotools.cocoeval"].COCOeval = object
    sys.path.insert(0, REF)
    from object_detection.utils import object_detection_evaluation

    gt, dt = make_set(np.random.RandomState(20261019))
    names = sorted({n for g in gt for s in g[3] for n in s.split("|")} - {""})
    ev = object_detection_evaluation.ObjectDetectionEvaluation(K, matching_iou_threshold=THR, subset_names=names)
    for i, ((gb, gc, gd, gs), (db, ds, dc)) in enumerate(zip(gt, dt)):
        subset = np.where(gd, "", np.asarray(gs, dtype=object)) if len(gs) else np.zeros(0, dtype=object)
        ev.add_single_ground_truth_image_info(i, gb, gc, list(subset))
        ev.add_single_detected_image_info(i, db, ds, dc)
    ap, mean_ap, _, _, corloc, mean_corloc = ev.evaluate()
    img = lambda parts: np.repeat(np.arange(len(parts)), [len(p[0]) for p in parts]).astype(np.int64)
    out = dict(
        gt_boxes=np.concatenate([g[0] for g in gt]), gt_classes=np.concatenate([g[1] for g in gt]).astype(np.int64),
        gt_difficult=np.concatenate([g[2] for g in gt]).astype(bool),
        gt_subset=np.asarray([s for g in gt for s in g[3]], dtype="U32"), gt_image=img(gt),
        dt_boxes=np.concatenate([d[0] for d in dt]), dt_scores=np.concatenate([d[1] for d in dt]),
        dt_classes=np.concatenate([d[2] for d in dt]).astype(np.int64), dt_image=img(dt),
        num_images=np.int64(N_IMG), num_classes=np.int64(K), iou_threshold=np.float64(THR),
        subset_names=np.asarray(names, dtype="U32"), ap=np.stack([ap[n] for n in names]),
        mean_ap=np.asarray([mean_ap[n] for n in names], np.float64),
        num_gt=np.stack([ev.num_gt_instances_per_class[n] for n in names]).astype(np.int64),
        corloc=np.asarray(corloc, np.float64), mean_corloc=np.float64(mean_corloc))
    path = os.path.join(HERE, "pascal_subset_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", dict(zip(names, out["mean_ap"])), "corloc", mean_corloc)
    print("num_gt", out["num_gt"].tolist(), "ap", np.round(out["ap"], 3).tolist())


if __name__ == "__main__":
    main()
