#!/usr/bin/env python3
"""Generate tests/golden/eval_nms_golden.npz: the reference evaluator's per-class NMS on seeded detection sets.

Run in the authoring container only (needs /root/reference):
    python tests/golden/make_eval_golden.py

For every case the reference's np_box_list_ops.non_max_suppression (nms_type 'standard') or
soft_non_max_suppression (2 = 'soft-linear', 3 = 'soft-gaussian') runs exactly as per_image_evaluation.py:35-68
wires it, on fp32 boxes promoted to float64 and multiplied by the case's scale (what the evaluator is handed) and
fp32 scores (all distinct: np.argsort is not stable). Stored, data only:
  c<i>_boxes [n,4] float32, c<i>_scores [n] float32, c<i>_scale [4] float64
  c<i>_index [m] int64   input indices of the returned boxes, in returned order
  c<i>_out   [m] float32 their returned scores
  cases [C,4] float64    (nms_type 1/2/3, iou_threshold, sigma, max_output_size)
"""
import builtins
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def detections(rng, n, scale):
    """n boxes around a few centres (so that IoUs span 0..1) with distinct fp32 scores in (0, 1]."""
    centres = rng.uniform(0.2, 0.8, (max(1, n // 6), 2))
    c = centres[rng.randint(0, len(centres), n)] + rng.normal(0, 0.04, (n, 2))
    hw = rng.uniform(0.05, 0.3, (n, 2))
    boxes = np.concatenate([c - hw / 2, c + hw / 2], 1).astype(np.float32)
    while True:
        scores = rng.uniform(0.001, 1.0, n).astype(np.float32)
        if len(np.unique(scores)) == n:
            return boxes, scores


def main():
    builtins.xrange = range                      # py2 idiom in np_box_list_ops.py:240,329,338
    sys.path.insert(0, REF)
    from object_detection.utils import np_box_list, np_box_list_ops

    rng = np.random.RandomState(20261016)
    out, cases = {}, []
    settings = [(1, 0.5, 0.5), (1, 0.3, 0.5), (1, 0.7, 0.5), (1, 1.0, 0.5),
                (2, 0.5, 0.5), (2, 0.3, 0.5), (2, 0.7, 0.5), (2, 1.0, 0.5),
                (3, 0.5, 0.5), (3, 0.3, 0.3), (3, 0.7, 0.5), (3, 0.5, 1.0), (3, 1.0, 0.5)]
    sizes = [(1, 10000), (7, 10000), (40, 10000), (120, 256), (300, 256), (300, 10000), (60, 5)]
    for t, thr, sigma in settings:
        for n, cap in sizes:
            scale = np.asarray([480.0, 640.0, 480.0, 640.0]) if len(cases) % 2 else np.ones(4)
            boxes, scores = detections(rng, n, scale)
            bl = np_box_list.BoxList(boxes.astype(np.float64) * scale)
            bl.add_field("scores", scores.copy())
            bl.add_field("index", np.arange(n))
            if t == 1:
                res = np_box_list_ops.non_max_suppression(bl, max_output_size=cap, iou_threshold=thr)
            else:
                res = np_box_list_ops.soft_non_max_suppression(bl, max_output_size=cap, iou_threshold=thr,
                                                               nms_type=t, sigma=sigma)
            i = len(cases)
            out["c%d_boxes" % i], out["c%d_scores" % i], out["c%d_scale" % i] = boxes, scores, scale
            out["c%d_index" % i] = np.asarray(res.get_field("index"), np.int64)
            out["c%d_out" % i] = np.asarray(res.get_field("scores"), np.float32)
            cases.append((t, thr, sigma, cap))
    out["cases"] = np.asarray(cases, np.float64)
    path = os.path.join(HERE, "eval_nms_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
