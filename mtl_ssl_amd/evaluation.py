"""PASCAL-VOC style detection evaluation: mAP at a matching IoU, CorLoc.

Restates the reference's numpy evaluator — utils/object_detection_evaluation.py:43-294
(ObjectDetectionEvaluation), utils/per_image_evaluation.py:28-281 (tp/fp labelling with "difficult"
boxes, CorLoc) and utils/metrics.py:21-127 (precision/recall, VOC-devkit average precision) — as a
small array-oriented module. Host-side numpy: the evaluator is outside the training hot path and
consumes the arrays `FasterRCNNMetaArch.postprocess` returns (after `.cpu()`).
"""
import numpy as np


def iou_matrix(a, b):
    """utils/np_box_ops.py:25-78: pairwise IoU of [N,4] and [M,4] boxes (ymin,xmin,ymax,xmax)."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    ih = np.maximum(0.0, np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]))
    iw = np.maximum(0.0, np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]))
    inter = ih * iw
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    return inter / (area_a[:, None] + area_b[None, :] - inter)


def precision_recall(scores, labels, num_gt):
    """metrics.compute_precision_recall (utils/metrics.py:21-67)."""
    scores, labels = np.asarray(scores), np.asarray(labels)
    if labels.dtype != bool or labels.ndim != 1:
        raise ValueError("tp/fp labels: expected a 1-D boolean array, got dtype %s with %d dimension(s)" % (labels.dtype, labels.ndim))
    if scores.ndim != 1:
        raise ValueError("detection scores: expected a 1-D array, got %d dimension(s)" % scores.ndim)
    if num_gt < labels.sum():
        raise ValueError("%d true positives but only %d groundtruth boxes of this class" % (int(labels.sum()), num_gt))
    if len(scores) != len(labels):
        raise ValueError("%d scores for %d tp/fp labels" % (len(scores), len(labels)))
    if num_gt == 0:
        return None, None
    order = np.argsort(scores)[::-1]
    tp = labels[order].astype(int)
    ctp, cfp = np.cumsum(tp), np.cumsum(1 - tp)
    return ctp.astype(float) / (ctp + cfp), ctp.astype(float) / num_gt


def average_precision(precision, recall):
    """metrics.compute_average_precision (utils/metrics.py:70-127): area under the
    monotonically-decreasing envelope of the precision/recall curve (VOC devkit, all points)."""
    if precision is None:
        if recall is not None:
            raise ValueError("a class without groundtruth has neither precision nor recall: got a recall array next to precision=None")
        return np.nan
    precision, recall = np.asarray(precision, float), np.asarray(recall, float)
    if len(precision) != len(recall):
        raise ValueError("precision has %d points, recall %d" % (len(precision), len(recall)))
    if not precision.size:
        return 0.0
    if precision.min() < 0 or precision.max() > 1:
        raise ValueError("precision values outside [0, 1]")
    if recall.min() < 0 or recall.max() > 1:
        raise ValueError("recall values outside [0, 1]")
    if np.any(np.diff(recall) < 0):
        raise ValueError("recall decreases along the curve (it must be non-decreasing)")
    r = np.concatenate([[0.0], recall, [1.0]])
    p = np.concatenate([[0.0], precision, [0.0]])
    p = np.maximum.accumulate(p[::-1])[::-1]
    idx = np.where(r[1:] != r[:-1])[0] + 1
    return float(np.sum((r[idx] - r[idx - 1]) * p[idx]))


class PascalDetectionEvaluator:
    """ObjectDetectionEvaluation with the 'default' subset: boxes flagged difficult are neither
    counted as groundtruth nor do detections matched to them count as true or false positives."""

    def __init__(self, num_classes, matching_iou_threshold=0.5, max_detections_per_class=10000):
        self.K, self.thr, self.cap = int(num_classes), float(matching_iou_threshold), int(max_detections_per_class)
        self.clear()

    def clear(self):
        self.gt = {}
        self.seen = set()
        self.num_gt = np.zeros(self.K, int)
        self.num_gt_imgs = np.zeros(self.K, int)
        self.scores = [[] for _ in range(self.K)]
        self.labels = [[] for _ in range(self.K)]
        self.correct_imgs = np.zeros(self.K)

    def add_single_ground_truth_image_info(self, image_key, boxes, class_labels, is_difficult=None):
        if image_key in self.gt:
            return
        boxes = np.asarray(boxes, float).reshape(-1, 4)
        cls = np.asarray(class_labels, int).reshape(-1)
        diff = np.zeros(len(cls), bool) if is_difficult is None else np.asarray(is_difficult, bool).reshape(-1)
        self.gt[image_key] = (boxes, cls, diff)
        for c in range(self.K):
            self.num_gt[c] += int(np.sum((cls == c) & ~diff))
            self.num_gt_imgs[c] += int(np.any(cls == c))

    def add_single_detected_image_info(self, image_key, boxes, scores, class_labels):
        boxes = np.asarray(boxes, float).reshape(-1, 4)
        scores = np.asarray(scores, float).reshape(-1)
        cls = np.asarray(class_labels, int).reshape(-1)
        if not (len(boxes) == len(scores) == len(cls)):
            raise ValueError("one image's detections disagree in length: %d boxes, %d scores, %d class labels"
                             % (len(boxes), len(scores), len(cls)))
        if image_key in self.seen:
            return
        self.seen.add(image_key)
        gb, gc, gd = self.gt.get(image_key, (np.zeros((0, 4)), np.zeros(0, int), np.zeros(0, bool)))
        valid = (boxes[:, 0] < boxes[:, 2]) & (boxes[:, 1] < boxes[:, 3])       # _remove_invalid_boxes
        boxes, scores, cls = boxes[valid], scores[valid], cls[valid]
        for c in range(self.K):
            db, ds = boxes[cls == c], scores[cls == c]
            s, lab = self._tp_fp(db, ds, gb[gc == c], gd[gc == c])
            self.scores[c].append(s)
            self.labels[c].append(lab)
            # CorLoc: the top-scoring detection of the class hits any groundtruth box of the class
            if len(db) and np.any(gc == c):
                top = int(np.argmax(ds))
                self.correct_imgs[c] += float(iou_matrix(db[top:top + 1], gb[gc == c]).max() >= self.thr)

    def _tp_fp(self, db, ds, gb, gdiff):
        """per_image_evaluation.py:233-281: detections in descending score order; each takes its
        best-IoU groundtruth box; a box can be claimed once; matches to difficult boxes are dropped."""
        if not len(db):
            return np.zeros(0, float), np.zeros(0, bool)
        order = np.argsort(ds)[::-1][: self.cap]
        db, ds = db[order], ds[order]
        if not len(gb):
            return ds, np.zeros(len(ds), bool)
        iou = iou_matrix(db, gb)
        best = iou.argmax(1)
        taken = np.zeros(len(gb), bool)
        tp = np.zeros(len(ds), bool)
        drop = np.zeros(len(ds), bool)
        for i, g in enumerate(best):
            if iou[i, g] >= self.thr:
                if gdiff[g]:
                    drop[i] = True
                elif not taken[g]:
                    tp[i] = taken[g] = True
        return ds[~drop], tp[~drop]

    def evaluate(self):
        """Returns dict(ap_per_class, mean_ap, precisions, recalls, corloc_per_class, mean_corloc)."""
        ap = np.full(self.K, np.nan)
        precisions, recalls = [], []
        for c in range(self.K):
            if self.num_gt[c] == 0:
                continue
            s = np.concatenate(self.scores[c]) if self.scores[c] else np.zeros(0)
            lab = np.concatenate(self.labels[c]) if self.labels[c] else np.zeros(0, bool)
            p, r = precision_recall(s, lab, self.num_gt[c])
            precisions.append(p)
            recalls.append(r)
            ap[c] = average_precision(p, r)
        with np.errstate(invalid="ignore", divide="ignore"):
            corloc = np.where(self.num_gt_imgs == 0, np.nan, self.correct_imgs / np.maximum(self.num_gt_imgs, 1))
        return dict(ap_per_class=ap, mean_ap=float(np.nanmean(ap)) if np.any(~np.isnan(ap)) else float("nan"),
                    precisions=precisions, recalls=recalls, corloc_per_class=corloc,
                    mean_corloc=float(np.nanmean(corloc)) if np.any(~np.isnan(corloc)) else float("nan"))


def evaluate_detections(detections, groundtruth, num_classes, image_hw=None, matching_iou_threshold=0.5):
    """Convenience wrapper for `postprocess` outputs: detections = dict of arrays (detection_boxes
    [B,T,4] normalised, detection_scores [B,T], detection_classes [B,T] 0-based, num_detections [B]);
    groundtruth = list of (boxes [G,4] normalised, classes [G] 0-based[, difficult [G]])."""
    ev = PascalDetectionEvaluator(num_classes, matching_iou_threshold)
    for i, g in enumerate(groundtruth):
        ev.add_single_ground_truth_image_info(i, g[0], g[1], g[2] if len(g) > 2 else None)
        n = int(detections["num_detections"][i])
        ev.add_single_detected_image_info(i, detections["detection_boxes"][i][:n], detections["detection_scores"][i][:n],
                                          detections["detection_classes"][i][:n])
    return ev.evaluate()


# ------------------------------------------------------------------------------ PASCAL groundtruth subsets
class PascalSubsetEvaluator:
    """ObjectDetectionEvaluation(subset_names=...) (utils/object_detection_evaluation.py:52-276, fed by
    eval_util.py:300-380): every groundtruth box carries a '|'-joined string of subset names and each subset gets its
    own PASCAL result — by definition what PascalDetectionEvaluator gives for the same images with is_difficult =
    ~member(subset). A box flagged difficult belongs to no subset (eval_util.py:343-350). CorLoc does not depend on the
    subset. The add_* methods only store; evaluate() does the work, in the order the detections were added.

    The subset only decides what a detection's best-IoU box means, not which box that is, so with a CUDA `device` the
    labelling of all subsets of all (image, class) pairs runs there in one launch (ops.pascal_match, pinned bit for bit
    against _tp_fp); device=None loops _tp_fp per subset. The accumulation after it is PascalDetectionEvaluator's own
    evaluate() on both paths.

    Unlike the reference, an image whose `subsets` disagree in length with its boxes, or that has none while other
    images have them, is an error naming the image (the reference falls back to a subset 'default' and then raises
    unless some box names it), and strings that are all empty give no subsets and a warning (the reference invents
    an empty 'default' whose mAP is NaN)."""
    MAX_DEVICE_SUBSETS = 64              # ops.PASCAL_MATCH_MAX_SUBSETS: one lane per subset; more stay on the host

    def __init__(self, num_classes, matching_iou_threshold=0.5, max_detections_per_class=10000, device=None):
        self._pascal = PascalDetectionEvaluator(num_classes, matching_iou_threshold, max_detections_per_class)
        self.K, self.thr, self.cap = self._pascal.K, self._pascal.thr, self._pascal.cap
        if device is not None:
            import torch
            device = torch.device(device)
            if device.type != "cuda":
                raise ValueError("PascalSubsetEvaluator: device %s is no CUDA device (None = the host path)" % device)
        self.device = device
        self.timings = {}
        self.clear()

    def clear(self):
        self.gt, self.dt = {}, {}

    def add_single_ground_truth_image_info(self, image_key, boxes, class_labels, is_difficult=None, subsets=None):
        if image_key in self.gt:
            return
        boxes = np.asarray(boxes, float).reshape(-1, 4)
        cls = np.asarray(class_labels, int).reshape(-1)
        diff = np.zeros(len(cls), bool) if is_difficult is None else np.asarray(is_difficult, bool).reshape(-1)
        if subsets is not None:
            subsets = [s.decode("utf-8") if isinstance(s, bytes) else str(s) for s in subsets]
            if len(subsets) != len(boxes):
                raise ValueError("image %r: %d subset strings for %d groundtruth boxes" % (image_key, len(subsets), len(boxes)))
        self.gt[image_key] = (boxes, cls, diff, subsets)

    def add_single_detected_image_info(self, image_key, boxes, scores, class_labels):
        boxes = np.asarray(boxes, float).reshape(-1, 4)
        scores = np.asarray(scores, float).reshape(-1)
        cls = np.asarray(class_labels, int).reshape(-1)
        if not (len(boxes) == len(scores) == len(cls)):
            raise ValueError("one image's detections disagree in length: %d boxes, %d scores, %d class labels"
                             % (len(boxes), len(scores), len(cls)))
        if image_key in self.dt:
            return
        valid = (boxes[:, 0] < boxes[:, 2]) & (boxes[:, 1] < boxes[:, 3])       # _remove_invalid_boxes
        self.dt[image_key] = (boxes[valid], scores[valid], cls[valid])

    def subset_names(self):
        """The union of the stored images' subset names, '' dropped, sorted. Raises when images with and without
        subset strings are mixed."""
        have = [k for k, g in self.gt.items() if g[3] is not None]
        if have and len(have) != len(self.gt):
            lacking = next(k for k, g in self.gt.items() if g[3] is None)
            raise ValueError("image %r has no groundtruth subsets, image %r has them: all images or none" % (lacking, have[0]))
        return sorted({n for k in have for s in self.gt[k][3] for n in s.split("|")} - {""})

    def _members(self, names):
        """{image key: bool [G, S]}: box g belongs to subset s; a difficult box belongs to none."""
        col = {n: j for j, n in enumerate(names)}
        out = {}
        for key, (boxes, cls, diff, subsets) in self.gt.items():
            m = np.zeros((len(boxes), len(names)), bool)
            for g, s in enumerate(subsets or ()):
                for n in s.split("|"):
                    if n:
                        m[g, col[n]] = True
            m[diff] = False
            out[key] = m
        return out

    def _segments(self, members):
        """(image key, class, detections of the class, their scores, the class's groundtruth boxes, their membership
        [G, S]) for every image with detections, in the order they were added, and every class."""
        S = next(iter(members.values())).shape[1] if members else 0
        none = (np.zeros((0, 4)), np.zeros(0, int))
        for key, (boxes, scores, cls) in self.dt.items():
            gb, gc = self.gt[key][:2] if key in self.gt else none
            mem = members.get(key, np.zeros((0, S), bool))
            for c in range(self.K):
                yield key, c, boxes[cls == c], scores[cls == c], gb[gc == c], mem[gc == c]

    def _labels_host(self, members, S):
        """scores / labels [S][K] lists of per-image arrays and the CorLoc hits [K], through _tp_fp once per subset."""
        scores = [[[] for _ in range(self.K)] for _ in range(S)]
        labels = [[[] for _ in range(self.K)] for _ in range(S)]
        correct = np.zeros(self.K)
        for key, c, db, ds, gb, mem in self._segments(members):
            for s in range(S):
                sc, lab = self._pascal._tp_fp(db, ds, gb, ~mem[:, s])
                scores[s][c].append(sc)
                labels[s][c].append(lab)
            if len(db) and len(gb):
                top = int(np.argmax(ds))
                correct[c] += float(iou_matrix(db[top:top + 1], gb).max() >= self.thr)
        return scores, labels, correct

    def _segment_tables(self, members, S):
        """What ops.pascal_match reads: every (image, class) pair with a detection, ordered by (class, image) so that a
        class's detections are one run of the flat arrays. Detections are sorted and capped by _tp_fp's own numpy calls
        (score ties fall as they fall there); top_pos = where the segment's np.argmax(ds) detection landed (-1: the cap
        cut it off); membership as one uint64 word per groundtruth box."""
        per_class = [[] for _ in range(self.K)]
        for key, c, db, ds, gb, mem in self._segments(members):
            if len(db):
                per_class[c].append((key, db, ds, gb, mem))
        weights = np.uint64(1) << np.arange(S, dtype=np.uint64)
        seg_key, seg_cat, dbs, dss, gbs, gms, tops, n_dt, n_gt = [], [], [], [], [], [], [], [], []
        for c, segs in enumerate(per_class):
            for key, db, ds, gb, mem in segs:
                order = np.argsort(ds)[::-1][: self.cap]
                pos = np.flatnonzero(order == int(np.argmax(ds)))
                seg_key.append(key)
                seg_cat.append(c)
                dbs.append(db[order])
                dss.append(ds[order])
                gbs.append(gb)
                gms.append((mem.astype(np.uint64) * weights[None, :]).sum(1, dtype=np.uint64))
                tops.append(int(pos[0]) if len(pos) else -1)
                n_dt.append(len(order))
                n_gt.append(len(gb))
        cat = lambda parts, shape, dtype: (np.concatenate(parts) if parts else np.zeros(0)).astype(dtype).reshape(shape)
        return dict(seg_key=seg_key, seg_cat=np.asarray(seg_cat, np.int64), top_pos=np.asarray(tops, np.int64),
                    dt_off=np.concatenate([[0], np.cumsum(n_dt)]).astype(np.int64),
                    gt_off=np.concatenate([[0], np.cumsum(n_gt)]).astype(np.int64),
                    dt_boxes=cat(dbs, (-1, 4), np.float64), dt_scores=cat(dss, (-1,), np.float64),
                    gt_boxes=cat(gbs, (-1, 4), np.float64), gt_member=cat(gms, (-1,), np.uint64))

    def match_on_device(self, members, S, timings=None):
        """tp / drop [S, ND] bool and hit [ND] bool of every segment in ONE ops.pascal_match launch and one copy back;
        a segment with more groundtruth boxes than the kernel holds goes through _tp_fp instead. timings (a dict)
        receives the seconds of the table build, the kernel and the copy."""
        import time

        import torch
        from . import ops
        t0 = time.perf_counter()
        tab = self._segment_tables(members, S)
        ND = len(tab["dt_boxes"])
        dt_off, gt_off, n_gt = tab["dt_off"], tab["gt_off"], np.diff(tab["gt_off"])
        large = np.flatnonzero(n_gt > ops.PASCAL_MATCH_MAX_GT)
        gkeep = np.ones(int(gt_off[-1]), bool)
        for s in large:                                    # the kernel sees such a segment without groundtruth
            gkeep[gt_off[s]:gt_off[s + 1]] = False
        dev_gt_off = np.concatenate([[0], np.cumsum(np.where(n_gt > ops.PASCAL_MATCH_MAX_GT, 0, n_gt))])
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        args = (up(tab["dt_boxes"]), up(tab["gt_boxes"][gkeep]), up(tab["gt_member"][gkeep].view(np.int64)))
        if timings is not None:
            torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        with torch.cuda.device(self.device):
            packed = ops.pascal_match(dt_off, dev_gt_off, *args, self.thr, S)[3]
        if timings is not None:
            torch.cuda.synchronize(self.device)
        t2 = time.perf_counter()
        host = packed.cpu().numpy()
        t3 = time.perf_counter()
        raw_hit = host[2 * ND:].view(np.uint8)[:ND]
        if ND and raw_hit.max() > 1:
            raise RuntimeError("pascal_match left a detection out (hit %d)" % int(raw_hit.max()))
        bits = np.arange(S, dtype=np.uint64).reshape(S, 1)
        one = np.uint64(1)
        tp = ((host[:ND].view(np.uint64)[None, :] >> bits) & one).astype(bool)
        drop = ((host[ND:2 * ND].view(np.uint64)[None, :] >> bits) & one).astype(bool)
        hit = raw_hit.astype(bool)
        for s in large:
            d0, d1, g0, g1 = dt_off[s], dt_off[s + 1], gt_off[s], gt_off[s + 1]
            db, gb, gm = tab["dt_boxes"][d0:d1], tab["gt_boxes"][g0:g1], tab["gt_member"][g0:g1]
            iou = iou_matrix(db, gb)
            best = iou.argmax(1)
            over = iou[np.arange(len(db)), best] >= self.thr
            hit[d0:d1] = over
            for j in range(S):
                member = ((gm >> np.uint64(j)) & one).astype(bool)
                taken = np.zeros(len(gb), bool)
                for i, g in enumerate(best):               # _tp_fp's loop on the rows the table already sorted
                    tp[j, d0 + i] = drop[j, d0 + i] = False
                    if over[i]:
                        if not member[g]:
                            drop[j, d0 + i] = True
                        elif not taken[g]:
                            tp[j, d0 + i] = taken[g] = True
        if timings is not None:
            timings.update(table_build_s=t1 - t0, kernel_s=t2 - t1, copy_s=t3 - t2)
        return tab, tp, drop, hit

    def _labels_device(self, members, S):
        """_labels_host's result from one device match: per class one run of the flat arrays, per subset one mask."""
        tab, tp, drop, hit = self.match_on_device(members, S, self.timings)
        dt_off, seg_cat = tab["dt_off"], tab["seg_cat"]
        first = np.searchsorted(seg_cat, np.arange(self.K + 1))          # segments are ordered by class
        scores = [[[] for _ in range(self.K)] for _ in range(S)]
        labels = [[[] for _ in range(self.K)] for _ in range(S)]
        for c in range(self.K):
            d0, d1 = dt_off[first[c]], dt_off[first[c + 1]]
            for s in range(S):
                keep = ~drop[s, d0:d1]
                scores[s][c].append(tab["dt_scores"][d0:d1][keep])
                labels[s][c].append(tp[s, d0:d1][keep])
        correct = np.zeros(self.K)
        has_gt = np.diff(tab["gt_off"]) > 0
        for i in np.flatnonzero(has_gt):
            pos = tab["top_pos"][i]
            if pos >= 0:
                correct[seg_cat[i]] += float(hit[dt_off[i] + pos])
            else:                                          # the cap cut the arg-max detection off: ask the host
                key, c = tab["seg_key"][i], int(seg_cat[i])
                boxes, sc, cls = self.dt[key]
                db, ds = boxes[cls == c], sc[cls == c]
                gb, gc = self.gt[key][:2]
                top = int(np.argmax(ds))
                correct[c] += float(iou_matrix(db[top:top + 1], gb[gc == c]).max() >= self.thr)
        return scores, labels, correct

    def evaluate(self):
        """-> dict(subset_names [S] sorted, ap_per_class {name: [K]}, mean_ap {name: float}, precisions / recalls
        {name: list of per-class arrays}, num_gt {name: [K]}, corloc_per_class [K], mean_corloc)."""
        import time
        import warnings
        names = self.subset_names()
        S = len(names)
        if not S:
            warnings.warn("PascalSubsetEvaluator: no groundtruth box names a subset: there are no subset metrics")
        members = self._members(names)
        self.timings = {}
        t0 = time.perf_counter()
        if self.device is None or S > self.MAX_DEVICE_SUBSETS or not S:
            scores, labels, correct = self._labels_host(members, S)
            self.timings["match_s"] = time.perf_counter() - t0
        else:
            scores, labels, correct = self._labels_device(members, S)
        t0 = time.perf_counter()
        num_gt_imgs = np.zeros(self.K, int)
        num_gt = np.zeros((S, self.K), int)
        for key, (boxes, cls, diff, subsets) in self.gt.items():
            for c in range(self.K):
                num_gt_imgs[c] += int(np.any(cls == c))
                num_gt[:, c] += members[key][cls == c].sum(0)
        out = dict(subset_names=names, ap_per_class={}, mean_ap={}, precisions={}, recalls={}, num_gt={})
        acc = self._pascal
        acc.clear()
        acc.num_gt_imgs, acc.correct_imgs = num_gt_imgs, correct
        for s, name in enumerate(names):                   # PascalDetectionEvaluator.evaluate() on this subset's lists
            acc.num_gt, acc.scores, acc.labels = num_gt[s], scores[s], labels[s]
            res = acc.evaluate()
            out["ap_per_class"][name], out["mean_ap"][name] = res["ap_per_class"], res["mean_ap"]
            out["precisions"][name], out["recalls"][name] = res["precisions"], res["recalls"]
            out["num_gt"][name] = num_gt[s].copy()
        acc.num_gt, acc.scores, acc.labels = np.zeros(self.K, int), [[] for _ in range(self.K)], [[] for _ in range(self.K)]
        res = acc.evaluate()
        out["corloc_per_class"], out["mean_corloc"] = res["corloc_per_class"], res["mean_corloc"]
        acc.clear()
        self.timings["accumulate_s"] = time.perf_counter() - t0
        return out


def macro_pr_curve(precisions, recalls):
    """eval_util.compute_pr_curve (eval_util.py:100-173): the macro-averaged precision/recall curve of the per-class
    curves. Classes without a curve (None) or with a single point are skipped; per class, equal recalls keep their
    highest precision and the precision becomes its running maximum from the high-recall end; then, for every distinct
    recall value of any class in descending order, the mean over the kept classes of the precision at the first point
    whose recall reaches it (a class that never reaches it adds 0). -> (precisions, recalls), recalls descending.
    PARITY UNPINNED: the reference's file imports TensorFlow and cannot be run next to this one."""
    if len(precisions) != len(recalls):
        raise ValueError("precision/recall number of class not matched")
    for p, r in zip(precisions, recalls):
        if p is not None and r is not None and len(p) != len(r):
            raise ValueError("precision/recall number of class not matched")
    new_p, new_r = [], []
    for p, r in zip(precisions, recalls):
        if p is None or r is None or len(p) <= 1:
            continue
        pm, rn = [float(p[0])], [float(r[0])]
        for i in range(1, len(p)):
            if r[i] != rn[-1]:
                pm.append(float(p[i]))
                rn.append(float(r[i]))
            else:
                pm[-1] = max(pm[-1], float(p[i]))
        top = 0.0
        for i in reversed(range(len(pm))):
            top = max(pm[i], top)
            pm[i] = top
        new_p.append(pm)
        new_r.append(rn)
    thresholds = sorted({v for r in new_r for v in r}, reverse=True)
    index = [len(r) for r in new_r]
    out_p, out_r = [], []
    for th in thresholds:
        total = 0.0
        for i, (p, r) in enumerate(zip(new_p, new_r)):
            while index[i] > 0 and r[index[i] - 1] >= th:
                index[i] -= 1
            if index[i] < len(r):
                total += p[index[i]]
        out_p.append(total / len(new_p))
        out_r.append(th)
    return out_p, out_r


def nms_string(nms_type, nms_iou_threshold, soft_nms_sigma):
    """'_'.join(eval_util.get_string_list_for_nms(...)) (eval_util.py:49-56): 'standard_1.0', 'soft-gaussian_0.5'."""
    if nms_type in ("standard", "soft-linear"):
        return "%s_%s" % (nms_type, str(nms_iou_threshold))
    if nms_type == "soft-gaussian":
        return "%s_%s" % (nms_type, str(soft_nms_sigma))
    raise ValueError("Cannot identify NMS type.")


def write_pr_curves(eval_dir, precisions, recalls, nms_type, nms_iou_threshold, soft_nms_sigma):
    """eval_util.visualize_pr_curve's text files (eval_util.py:186-203): <eval_dir>/pr_curve_<subset>_<nms str>.txt, one
    '%f\\t%f\\n' line (precision, recall) per point of macro_pr_curve; precisions / recalls as evaluate() returns
    them. The matplotlib image summary is not written. Returns the paths."""
    import os
    tail = nms_string(nms_type, nms_iou_threshold, soft_nms_sigma)
    paths = []
    for name in precisions:
        p, r = macro_pr_curve(precisions[name], recalls[name])
        path = os.path.join(eval_dir, "pr_curve_" + name + "_" + tail + ".txt")
        with open(path, "w") as fh:
            for a, b in zip(p, r):
                fh.write("%f\t%f\n" % (a, b))
        paths.append(path)
    return paths


# ------------------------------------------------------------------------------ MS-COCO metrics
class CocoDetectionEvaluator:
    """The 12 MS-COCO box metrics of `eval_util.evaluate_detection_results_coco` (eval_util.py:393-550) /
    `CocoEvaluation` (utils/object_detection_evaluation.py:294-425).

    The reference collects, per image, the detections of all classes sorted by score, keeps the best 100
    (`max_detections_per_image`), converts boxes to [x, y, w, h] with category id = class + 1, and hands
    them to pycocotools' `COCOeval` (a third-party dependency that is absent here and from
    /root/reference; pinned by the reference to whatever `pip install pycocotools` gave in 2018, i.e.
    cocoapi 2.0). This class restates that published bbox algorithm in numpy — PARITY UNPINNED against
    pycocotools itself; the tests hold hand-derived known answers:

    * IoU thresholds .50:.05:.95, 101 recall thresholds, maxDets (1, 10, 100), area ranges all / small
      (< 32^2) / medium / large (>= 96^2) on the groundtruth (and unmatched detection) box areas;
    * per image and category, detections in descending score (stable) claim the unmatched groundtruth box
      of highest IoU >= threshold; crowd boxes can be claimed repeatedly (IoU against a crowd box is
      intersection over DETECTION area) and, like groundtruth outside the area range, make the detection
      "ignored" instead of true/false positive; regular boxes are preferred over ignored ones;
    * precision is made monotonically non-increasing and sampled at the recall thresholds; AP / AR are the
      means over the entries that exist (-1 where a category has no groundtruth).

    `_iou` and `_evaluate_image` define the match. With a CUDA `device` evaluate() runs it there instead
    (ops.coco_match, one launch for all images and categories, pinned bit for bit against these two
    functions); the accumulation after it is the same host code on both paths.
    """
    IOU_THRS = np.linspace(0.5, 0.95, 10)
    REC_THRS = np.linspace(0.0, 1.0, 101)
    MAX_DETS = (1, 10, 100)
    AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
    NAMES = ("AP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large",
             "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large")

    def __init__(self, num_classes, max_detections_per_image=100, device=None):
        """device: a CUDA device runs the greedy match of evaluate() there (ops.coco_match: every (image, category)
        pair in one launch, bit for bit what _evaluate_image gives); None keeps the numpy loops."""
        self.K, self.cap = int(num_classes), int(max_detections_per_image)
        if device is not None:
            import torch
            device = torch.device(device)
            if device.type != "cuda":
                raise ValueError("CocoDetectionEvaluator: device %s is no CUDA device (None = the host path)" % device)
        self.device = device
        self.timings = {}
        self.clear()

    def clear(self):
        self.gt, self.dt = {}, {}

    def add_single_ground_truth_image_info(self, image_key, boxes, class_labels, is_crowd=None, areas=None):
        """boxes [G,4] (ymin,xmin,ymax,xmax) in PIXELS (the area ranges are in pixels), classes 0-based."""
        if image_key in self.gt:
            return
        b = np.asarray(boxes, np.float64).reshape(-1, 4)
        c = np.asarray(class_labels, int).reshape(-1)
        crowd = np.zeros(len(c), bool) if is_crowd is None else np.asarray(is_crowd, bool).reshape(-1)
        a = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) if areas is None else np.asarray(areas, np.float64).reshape(-1)
        self.gt[image_key] = (b, c, crowd, a)

    def add_single_detected_image_info(self, image_key, boxes, scores, class_labels):
        b = np.asarray(boxes, np.float64).reshape(-1, 4)
        s = np.asarray(scores, np.float64).reshape(-1)
        c = np.asarray(class_labels, int).reshape(-1)
        if not (len(b) == len(s) == len(c)):
            raise ValueError("one image's detections disagree in length: %d boxes, %d scores, %d class labels"
                             % (len(b), len(s), len(c)))
        if image_key in self.dt:
            return
        valid = (b[:, 0] < b[:, 2]) & (b[:, 1] < b[:, 3])                # _remove_invalid_boxes
        b, s, c = b[valid], s[valid], c[valid]
        order = np.argsort(-s, kind="stable")[: self.cap]                # best 100 of the image, all classes
        self.dt[image_key] = (b[order], s[order], c[order])

    @staticmethod
    def _iou(d, g, crowd):
        ih = np.maximum(0.0, np.minimum(d[:, None, 2], g[None, :, 2]) - np.maximum(d[:, None, 0], g[None, :, 0]))
        iw = np.maximum(0.0, np.minimum(d[:, None, 3], g[None, :, 3]) - np.maximum(d[:, None, 1], g[None, :, 1]))
        inter = ih * iw
        ad = ((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1]))[:, None]
        ag = ((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[None, :]
        union = np.where(crowd[None, :], ad, ad + ag - inter)
        return inter / np.maximum(union, 1e-300)

    def _evaluate_image(self, key, cat, rng, max_det):
        gb, gc, gcrowd, garea = self.gt.get(key, (np.zeros((0, 4)), np.zeros(0, int), np.zeros(0, bool), np.zeros(0)))
        db, ds, dc = self.dt.get(key, (np.zeros((0, 4)), np.zeros(0), np.zeros(0, int)))
        gsel, dsel = gc == cat, dc == cat
        gb, gcrowd, garea = gb[gsel], gcrowd[gsel], garea[gsel]
        db, ds = db[dsel][:max_det], ds[dsel][:max_det]
        if not len(gb) and not len(db):
            return None
        gig = gcrowd | (garea < rng[0]) | (garea > rng[1])
        gorder = np.argsort(gig, kind="stable")                           # regular boxes first
        gb, gcrowd, gig = gb[gorder], gcrowd[gorder], gig[gorder]
        ious = self._iou(db, gb, gcrowd) if len(db) and len(gb) else np.zeros((len(db), len(gb)))
        T = len(self.IOU_THRS)
        gtm = np.zeros((T, len(gb)), bool)
        dtm = np.zeros((T, len(db)), bool)
        dig = np.zeros((T, len(db)), bool)
        for ti, t in enumerate(self.IOU_THRS):
            for di in range(len(db)):
                best, m = min(t, 1 - 1e-10), -1
                for gi in range(len(gb)):
                    if gtm[ti, gi] and not gcrowd[gi]:
                        continue
                    if m > -1 and not gig[m] and gig[gi]:
                        break
                    if ious[di, gi] < best:
                        continue
                    best, m = ious[di, gi], gi
                if m == -1:
                    continue
                dig[ti, di], dtm[ti, di], gtm[ti, m] = gig[m], True, True
        darea = (db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1])
        dig |= (~dtm) & ((darea < rng[0]) | (darea > rng[1]))[None, :]
        return ds, dtm, dig, int(np.sum(~gig))

    def _accumulate(self, scores, dtm, dig, npig):
        """One (category, area range, maxDets) cell: the detections of every image in image order with their dtm / dig
        [T,n] -> (recall [T], precision [T,R]) (COCOeval.accumulate)."""
        T, R = len(self.IOU_THRS), len(self.REC_THRS)
        rec, prec = np.zeros(T), np.zeros((T, R))
        order = np.argsort(-scores, kind="mergesort")
        dtm, dig = dtm[:, order], dig[:, order]
        tps = np.cumsum(dtm & ~dig, 1).astype(float)
        fps = np.cumsum(~dtm & ~dig, 1).astype(float)
        for t in range(T):
            tp, fp = tps[t], fps[t]
            rc = tp / npig
            pr = tp / (fp + tp + np.spacing(1))
            rec[t] = rc[-1] if len(tp) else 0
            pr = np.maximum.accumulate(pr[::-1])[::-1]
            inds = np.searchsorted(rc, self.REC_THRS, side="left")
            q = np.zeros(R)
            ok = inds < len(pr)
            q[ok] = pr[inds[ok]]
            prec[t] = q
        return rec, prec

    def _cells_host(self, keys):
        """(k, a, m, scores, dtm, dig, npig) of every cell that has an image, through _evaluate_image."""
        for k in range(self.K):
            for a, rng in enumerate(self.AREA_RNG):
                for m, md in enumerate(self.MAX_DETS):
                    res = [r for r in (self._evaluate_image(key, k, rng, md) for key in keys) if r is not None]
                    if not res:
                        continue
                    yield (k, a, m, np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res], 1),
                           np.concatenate([r[2] for r in res], 1), sum(r[3] for r in res))

    def _segment_tables(self, keys):
        """The (image, category) pairs that hold a detection or a groundtruth box, ordered by (category, image): their
        detections (in the image's descending-score order) and groundtruth boxes (input order) as flat arrays with
        offsets — what ops.coco_match reads. Classes outside [0, K) belong to no category, as on the host path."""
        none_g = (np.zeros((0, 4)), np.zeros(0, int), np.zeros(0, bool), np.zeros(0))
        none_d = (np.zeros((0, 4)), np.zeros(0), np.zeros(0, int))
        gts, dts = [self.gt.get(key, none_g) for key in keys], [self.dt.get(key, none_d) for key in keys]
        N = max(len(keys), 1)
        cat = lambda parts, j, dtype: (np.concatenate([p[j] for p in parts]) if parts else np.zeros(0)).astype(dtype)
        img = lambda parts: np.repeat(np.arange(len(parts)), [len(p[1]) for p in parts]).astype(np.int64)
        gb, gc, gcrowd, garea = (np.concatenate([p[0] for p in gts]).reshape(-1, 4) if gts else np.zeros((0, 4)),
                                 cat(gts, 1, np.int64), cat(gts, 2, bool), cat(gts, 3, np.float64))
        db, ds, dc = (np.concatenate([p[0] for p in dts]).reshape(-1, 4) if dts else np.zeros((0, 4)),
                      cat(dts, 1, np.float64), cat(dts, 2, np.int64))
        gkey, dkey = gc * N + img(gts), dc * N + img(dts)
        gsel = np.flatnonzero((gc >= 0) & (gc < self.K))
        dsel = np.flatnonzero((dc >= 0) & (dc < self.K))
        gsel = gsel[np.argsort(gkey[gsel], kind="stable")]
        dsel = dsel[np.argsort(dkey[dsel], kind="stable")]
        seg_key = np.unique(np.concatenate([gkey[gsel], dkey[dsel]]))
        S = len(seg_key)
        off = lambda k: np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(seg_key, k), minlength=S))])
        return dict(seg_cat=seg_key // N, seg_img=seg_key % N, dt_off=off(dkey[dsel]), gt_off=off(gkey[gsel]),
                    dt_boxes=np.ascontiguousarray(db[dsel]), dt_scores=ds[dsel], gt_boxes=np.ascontiguousarray(gb[gsel]),
                    gt_area=garea[gsel], gt_crowd=gcrowd[gsel])

    def match_on_device(self, keys, timings=None):
        """dtm / dig [T,A,ND] bool and npig [S,A] of every segment in ONE ops.coco_match launch and one copy back; a
        segment with more groundtruth boxes than the kernel holds goes through _evaluate_image instead. timings (a
        dict) receives the seconds of the table build, the kernel and the copy."""
        import time

        import torch
        from . import ops
        T, A = len(self.IOU_THRS), len(self.AREA_RNG)
        t0 = time.perf_counter()
        tab = self._segment_tables(keys)
        S, ND = len(tab["seg_cat"]), len(tab["dt_boxes"])
        gt_off, n_gt = tab["gt_off"], np.diff(tab["gt_off"])
        large = np.flatnonzero(n_gt > ops.COCO_MATCH_MAX_GT)
        gkeep = np.ones(int(gt_off[-1]), bool)
        for s in large:                                    # the kernel sees such a segment without groundtruth
            gkeep[gt_off[s]:gt_off[s + 1]] = False
        dev_gt_off = np.concatenate([[0], np.cumsum(np.where(n_gt > ops.COCO_MATCH_MAX_GT, 0, n_gt))])
        up = lambda x, dtype: torch.from_numpy(np.ascontiguousarray(x, dtype)).to(self.device)
        args = (up(tab["dt_boxes"], np.float64), up(tab["gt_boxes"][gkeep], np.float64),
                up(tab["gt_area"][gkeep], np.float64), up(tab["gt_crowd"][gkeep], np.uint8),
                up(self.IOU_THRS, np.float64), up(np.asarray(self.AREA_RNG), np.float64))
        if timings is not None:
            torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        with torch.cuda.device(self.device):
            packed = ops.coco_match(tab["dt_off"], dev_gt_off, *args)[3]
        if timings is not None:
            torch.cuda.synchronize(self.device)
        t2 = time.perf_counter()
        host = packed.cpu().numpy()
        t3 = time.perf_counter()
        bits = np.arange(T * A, dtype=np.uint64).reshape(T, A, 1)
        one = np.uint64(1)
        dtm = ((host[:ND].view(np.uint64)[None, None, :] >> bits) & one).astype(bool)
        dig = ((host[ND:2 * ND].view(np.uint64)[None, None, :] >> bits) & one).astype(bool)
        npig = host[2 * ND:].view(np.int32)[:S * A].reshape(S, A).astype(np.int64)
        if S and npig.min() < 0:
            raise RuntimeError("coco_match left a segment out (npig %d)" % int(npig.min()))
        for s in large:
            d0, d1 = tab["dt_off"][s], tab["dt_off"][s + 1]
            for a, rng in enumerate(self.AREA_RNG):
                _, m, g, n = self._evaluate_image(keys[tab["seg_img"][s]], int(tab["seg_cat"][s]), rng, d1 - d0)
                dtm[:, a, d0:d1], dig[:, a, d0:d1], npig[s, a] = m, g, n
        if timings is not None:
            timings.update(table_build_s=t1 - t0, kernel_s=t2 - t1, copy_s=t3 - t2)
        return tab, dtm, dig, npig

    def _cells_device(self, keys):
        """The cells of _cells_host from one device match: the first m detections of a segment are its maxDets = m
        result (whether a detection matches depends only on the detections before it)."""
        tab, dtm, dig, npig = self.match_on_device(keys, self.timings)
        dt_off, seg_cat = tab["dt_off"], tab["seg_cat"]
        rank = np.arange(int(dt_off[-1])) - np.repeat(dt_off[:-1], np.diff(dt_off))
        first = np.searchsorted(seg_cat, np.arange(self.K + 1))          # segments are ordered by category
        for k in range(self.K):
            s0, s1 = first[k], first[k + 1]
            if s0 == s1:
                continue
            d0, d1 = dt_off[s0], dt_off[s1]
            for a in range(len(self.AREA_RNG)):
                for m, md in enumerate(self.MAX_DETS):
                    sel = rank[d0:d1] < md
                    yield (k, a, m, tab["dt_scores"][d0:d1][sel], dtm[:, a, d0:d1][:, sel], dig[:, a, d0:d1][:, sel],
                           int(npig[s0:s1, a].sum()))

    def evaluate(self):
        """-> dict(stats = the 12 COCO numbers in pycocotools' order, by name too, per_class_ap [K], per_class_stats
        [K,12] = the 12 numbers with the category axis restricted to one category)."""
        import time
        T, R, A, M = len(self.IOU_THRS), len(self.REC_THRS), len(self.AREA_RNG), len(self.MAX_DETS)
        precision = -np.ones((T, R, self.K, A, M))
        recall = -np.ones((T, self.K, A, M))
        keys = sorted(set(self.gt) | set(self.dt), key=str)
        self.timings = {}
        cells = self._cells_host(keys) if self.device is None else self._cells_device(keys)
        spent = 0.0
        for k, a, m, scores, dtm, dig, npig in cells:
            if npig == 0:
                continue
            t0 = time.perf_counter()
            recall[:, k, a, m], precision[:, :, k, a, m] = self._accumulate(scores, dtm, dig, npig)
            spent += time.perf_counter() - t0
        self.timings["accumulate_s"] = spent

        def mean_valid(x):
            x = x[x > -1]
            return float(x.mean()) if x.size else -1.0

        def twelve(precision, recall):
            def ap(iou=None, area=0, md=2):
                p = precision if iou is None else precision[np.isclose(self.IOU_THRS, iou)]
                return mean_valid(p[:, :, :, area, md])

            def ar(area=0, md=2):
                return mean_valid(recall[:, :, area, md])

            return [ap(), ap(0.5), ap(0.75), ap(area=1), ap(area=2), ap(area=3),
                    ar(md=0), ar(md=1), ar(md=2), ar(area=1), ar(area=2), ar(area=3)]

        stats = twelve(precision, recall)
        out = dict(zip(self.NAMES, stats))
        out["stats"] = np.asarray(stats)
        out["per_class_ap"] = np.asarray([mean_valid(precision[:, :, k, 0, 2]) for k in range(self.K)])
        out["per_class_stats"] = np.asarray([twelve(precision[:, :, k:k + 1], recall[:, k:k + 1])
                                             for k in range(self.K)]).reshape(self.K, 12)
        return out


def evaluate_detections_coco(detections, groundtruth, num_classes, image_hw):
    """`postprocess` outputs (normalised boxes) + groundtruth list of (boxes normalised [G,4], classes [G]
    0-based[, is_crowd [G]]) + image size (H, W) in pixels -> CocoDetectionEvaluator.evaluate()."""
    H, W = image_hw
    scale = np.asarray([H, W, H, W], np.float64)
    ev = CocoDetectionEvaluator(num_classes)
    for i, g in enumerate(groundtruth):
        ev.add_single_ground_truth_image_info(i, np.asarray(g[0], np.float64).reshape(-1, 4) * scale, g[1],
                                              g[2] if len(g) > 2 else None)
        n = int(detections["num_detections"][i])
        ev.add_single_detected_image_info(i, np.asarray(detections["detection_boxes"][i][:n], np.float64) * scale,
                                          detections["detection_scores"][i][:n], detections["detection_classes"][i][:n])
    return ev.evaluate()
