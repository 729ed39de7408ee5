"""The multi-task metrics of the evaluator: `get_mtl_metrics` (utils/mtl_util.py:20-107), merged into the metrics at
eval_util.py:853-860 as `mtl/window_map`, `mtl/closeness_diff` and `mtl/edgemask_ap`.

Host-side numpy over the few small arrays the evaluator copies back per image (window and closeness logits); the
edge-mask metric's per-pixel work runs on the device (ops.edgemask_agreement) and arrives here as one count.

What the reference does and this module reproduces on purpose:

* window: per window, softmax of the logits (in their fp32) as scores and `label > 0` as true positives, AP by
  metrics.compute_precision_recall / compute_average_precision; the mean over an image's windows, then over images.
  A window without a positive label has AP NaN, and so has the mean.
* closeness: each groundtruth box selects the detection slot of largest INTERSECTION (not IoU) with it, among the
  padded `max_total_detections` slots in absolute coordinates (0 when nothing intersects), and that slot index picks
  a row of the per-PROPOSAL closeness logits — the row of proposal i, not of the proposal that produced detection i.
  Sigmoid, rows with an all-zero label skipped, hit = argmax(dt[1:]) == argmax(gt[1:]); the mean per image, then over
  the images that have rows (0.0 if none).
* edge mask: the agreement of the resized prediction's label with channel 0 of the groundtruth mask, per image
  divided by h * w, then the mean over images.

Deviation: an image without windows is skipped by the window metric (the reference's empty mean makes the whole
metric NaN), and a slot index beyond the closeness rows is a ValueError (the reference raises IndexError).
"""
import numpy as np

from .evaluation import average_precision, precision_recall


def softmax(x):
    """mtl_util._softmax: in the dtype of x."""
    y = x - np.expand_dims(np.max(x, axis=-1), -1)
    y = np.exp(y)
    return y / np.expand_dims(np.sum(y, axis=-1), -1)


def sigmoid(x):
    """mtl_util._sigmoid: in the dtype of x."""
    return 1 / (1 + np.exp(-1.0 * x))


def intersection(boxes1, boxes2):
    """np_box_ops.intersection (utils/np_box_ops.py:37-60): pairwise intersection areas [N,M]."""
    y_min1, x_min1, y_max1, x_max1 = np.split(boxes1, 4, axis=1)
    y_min2, x_min2, y_max2, x_max2 = np.split(boxes2, 4, axis=1)
    ih = np.maximum(np.zeros((len(boxes1), len(boxes2))),
                    np.minimum(y_max1, np.transpose(y_max2)) - np.maximum(y_min1, np.transpose(y_min2)))
    iw = np.maximum(np.zeros((len(boxes1), len(boxes2))),
                    np.minimum(x_max1, np.transpose(x_max2)) - np.maximum(x_min1, np.transpose(x_min2)))
    return ih * iw


def window_image_map(window_logits, window_labels):
    """One image: mean over its windows of the AP of softmax(logits) against labels > 0; None without windows."""
    logits = np.asarray(window_logits)
    labels = np.asarray(window_labels, np.float32)
    if len(labels) == 0:
        return None
    if logits.shape != labels.shape:
        raise ValueError("window logits %s against window labels %s" % (logits.shape, labels.shape))
    aps = []
    for dt, gt in zip(logits, labels):
        tp = np.asarray(gt > 0, bool)
        p, r = precision_recall(softmax(dt), tp, int(np.sum(tp.astype(np.int32))))
        aps.append(average_precision(p, r))
    return float(np.mean(aps))


def closeness_slots(gt_boxes_abs, detection_boxes_abs):
    """The reference's gt -> detection-slot index: argmax over the padded slots of the intersection."""
    gt = np.asarray(gt_boxes_abs).reshape(-1, 4)
    dt = np.asarray(detection_boxes_abs).reshape(-1, 4)
    if not len(gt):
        return np.zeros(0, np.int64)
    return np.argmax(intersection(gt, dt), axis=1)


def closeness_image_hits(closeness_logits, closeness_labels, slots):
    """One image: the hit list (1.0 / 0.0 per groundtruth row with a non-zero label)."""
    logits = np.asarray(closeness_logits)
    hits = []
    for gt, s in zip(np.asarray(closeness_labels, np.float32), slots):
        if s >= len(logits):
            raise ValueError("closeness metric: groundtruth box matched detection slot %d, but the closeness head has "
                             "only %d rows (one per proposal): the reference indexes the per-proposal logits with the "
                             "detection slot (mtl_util.py:76-80), so max_total_detections must not exceed "
                             "first_stage_max_proposals" % (s, len(logits)))
        if int(np.sum(gt != 0)) == 0:
            continue
        dt = sigmoid(logits[s])
        hits.append(float(np.argmax(dt[1:]) == np.argmax(gt[1:])))
    return hits


class MtlMetrics:
    """Per-image accumulation of the three metrics; evaluate() gives the keys that saw any image."""

    def __init__(self):
        self.window, self.closeness, self.edgemask = [], [], []
        self.seen = set()

    def add_window(self, window_logits, window_labels):
        self.seen.add("window")
        m = window_image_map(window_logits, window_labels)
        if m is not None:
            self.window.append(m)

    def add_closeness(self, closeness_logits, closeness_labels, gt_boxes_abs, detection_boxes_abs):
        self.seen.add("closeness")
        hits = closeness_image_hits(closeness_logits, closeness_labels,
                                    closeness_slots(gt_boxes_abs, detection_boxes_abs))
        if hits:
            self.closeness.append(float(np.mean(hits)))

    def add_edgemask(self, agreement_count, h, w):
        self.seen.add("edgemask")
        self.edgemask.append(float(agreement_count) / float(int(h) * int(w)))

    def evaluate(self):
        out = {}
        if "window" in self.seen:
            out["mtl/window_map"] = float(np.mean(self.window)) if self.window else float("nan")
        if "closeness" in self.seen:
            out["mtl/closeness_diff"] = float(np.mean(self.closeness)) if self.closeness else 0.0
        if "edgemask" in self.seen:
            out["mtl/edgemask_ap"] = float(np.mean(self.edgemask)) if self.edgemask else 0.0
        return out
