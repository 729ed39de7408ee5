"""Evaluation launcher with the flags of object_detection/eval.py:66-82: restores the newest state of
--checkpoint_dir into an inference replica, runs predict -> (refine) -> postprocess over eval_input_reader's records
(evaluator.py:102-230: one image per step, at its own resized shape) and reports the metrics of
eval_config.metrics_set (PASCAL VOC mAP at eval_config.iou_threshold by default, COCO mAP with 'coco_metrics').
With mtl.window / closeness / edgemask the model also gets the record's groundtruth windows and the JSON carries
mtl/window_map, mtl/closeness_diff and mtl/edgemask_ap (mtl_metrics.py); eval_config.nms_type / nms_threshold /
soft_nms_sigma re-suppress each class's detections on the device before the evaluator sees them
(utils/per_image_evaluation.py:35-68, 258).
With 'coco_metrics' the evaluator's greedy match runs on the device (ops.coco_match), and eval_config.coco_eval_options
adds the COCO_Eval/<class>/<metric> keys it selects and may name an annotation file as the groundtruth
(eval_util.py:489-549).
Records that carry image/object/subset (create_pascal_tf_record --subsets) add one PASCAL result per groundtruth subset,
'Subset <name> mAP@<thr>IOU[/<category>]', labelled on the device (ops.pascal_match), and with --eval_dir the
pr_curve_<subset>_<nms>.txt files (eval_util.py:186-203, 300-380).
eval_config.calc_loss adds the model's losses (Loss/<name>, FasterRCNNMetaArch.eval_loss on the device);
submission_format_output writes the test servers' files instead of metrics; a metrics run with --eval_dir keeps the
best state under <eval_dir>/best/ (main_subset); --run_once=false evaluates every new state of --checkpoint_dir
(eval_interval_secs, max_evals) with the model built once; num_visualizations / visualization_export_dir export
annotated images (mtl_ssl_amd/eval_workflow.py). A metrics run with --eval_dir also leaves a TensorBoard event file there:
one scalar per metric at the state's global step and one image per visualisation (mtl_ssl_amd/summaries.py).

    python -m mtl_ssl_amd.eval --checkpoint_dir=/runs/a --eval_dir=/runs/a/eval --pipeline_config_path=..."""
import argparse
import json
import os
import sys
import warnings

import numpy as np


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return v


def eval_nms_options(ec):
    """(nms_type, nms_threshold, soft_nms_sigma, iou_threshold) of eval_config, as the float32 values the proto holds.
    An unknown nms_type is a ValueError (eval_util.get_string_list_for_nms)."""
    from .ops import EVAL_NMS_TYPES
    nms_type = str(ec.get("nms_type", "standard"))
    if nms_type not in EVAL_NMS_TYPES:
        raise ValueError("eval_config.nms_type %r: Cannot identify NMS type (standard, soft-linear or soft-gaussian)"
                         % nms_type)
    f32 = lambda v: float(np.float32(v))
    return (nms_type, f32(ec.get("nms_threshold", 1.0)), f32(ec.get("soft_nms_sigma", 0.5)),
            f32(ec.get("iou_threshold", 0.5)))


# eval_util.py:489-492: the reference's names of the twelve COCO numbers, in pycocotools' order
COCO_METRIC_NAMES = ("AP", "AP_IoU50", "AP_IoU75", "AP_small", "AP_medium", "AP_large",
                     "AR_max1", "AR_max10", "AR_max100", "AR_small", "AR_medium", "AR_large")


def coco_eval_options(ec):
    """eval_config.coco_eval_options (eval_util.py:495-522) -> None without the message, else dict(metric_index = the
    chosen rows of the twelve, in ascending order; class_type 0 = the row 'All', 1 = 'All' and every category;
    ann_filename = the annotation file when the config names one, else None). The two ValueErrors are the
    reference's."""
    from . import config
    opts = ec.get("coco_eval_options")
    if opts is None:
        return None
    if not isinstance(opts, config.Msg):
        raise ValueError("eval_config.coco_eval_options: a message expected, got %r" % (opts,))
    opts.kind = "CocoEvalOptions"
    index = [int(v) for v in opts.eval_metric_index] or [0]
    if min(index) < 0 or max(index) > len(COCO_METRIC_NAMES) - 1:
        raise ValueError("eval_metric_index")
    class_type = int(opts.eval_class_type)
    if class_type < 0 or class_type > 1:
        raise ValueError("eval_class_type")
    ann = str(opts.eval_ann_filename) if opts.has("eval_ann_filename") else ""
    return dict(metric_index=sorted(set(index)), class_type=class_type, ann_filename=ann or None)


def coco_class_names(num_classes, label_map_path=""):
    """{category id 1..K: name} of the COCO_Eval rows: the names of label_map_path — a category the map does not name
    has no row (eval_util.py:534-537) — or 'category_<id>' for every category without a map."""
    if not label_map_path:
        return {i: "category_%d" % i for i in range(1, int(num_classes) + 1)}
    from .create_pascal_tf_record import read_label_map
    names = {int(i): n for n, i in read_label_map(label_map_path).items()}
    return {i: names[i] for i in range(1, int(num_classes) + 1) if i in names}


def coco_eval_keys(res, options, class_names):
    """eval_util.py:519-547: {'COCO_Eval/<class name>/<metric name>': value} from CocoDetectionEvaluator.evaluate()'s
    stats (the row 'All', always first) and per_class_stats (one row per named category with class_type 1)."""
    rows = [("All", res["stats"])]
    if options["class_type"] == 1:
        rows += [(class_names[k + 1], res["per_class_stats"][k]) for k in range(len(res["per_class_stats"]))
                 if k + 1 in class_names]
    return {"COCO_Eval/%s/%s" % (name, COCO_METRIC_NAMES[i]): float(row[i])
            for name, row in rows for i in options["metric_index"]}


def pascal_subset_keys(res, iou_threshold, class_names):
    """eval_util.py:372-380: {'Subset <name> mAP@<thr>IOU': mAP, '.../<category>': AP} from
    PascalSubsetEvaluator.evaluate(), the name padded to ten columns as the reference formats it; a category that
    class_names (coco_class_names) does not hold has no key. The mAP keys come first, subsets in sorted order."""
    head = {name: "Subset {:10} mAP@{}IOU".format(name, iou_threshold) for name in res["subset_names"]}
    out = {head[name]: float(res["mean_ap"][name]) for name in res["subset_names"]}
    for name in res["subset_names"]:
        for k, v in enumerate(res["ap_per_class"][name]):
            if k + 1 in class_names:
                out["%s/%s" % (head[name], class_names[k + 1])] = float(v)
    return out


class CocoAnnotations:
    """Groundtruth of the COCO evaluator from an instances JSON (coco_eval_options.eval_ann_filename), which holds what
    the records do not: crowd flags and segmentation areas. Only the images that are evaluated count (the reference
    evaluates against every image of the file)."""

    def __init__(self, path):
        from .create_mscoco_tf_record import read_instances
        ann, _, self.per_image = read_instances(path)
        self.path = path
        self.images = {int(i["id"]): i for i in ann.get("images", [])}

    def image(self, source_id):
        """image/source_id of a record -> (integer image id, (height, width) in pixels of the original image, boxes
        [G,4] (ymin, xmin, ymax, xmax) in those pixels, classes 0-based = category_id - 1, iscrowd, area)."""
        try:
            image_id = int(source_id)
        except (TypeError, ValueError):
            image_id = None
        if image_id not in self.images:
            raise ValueError("evaluated image %r (image/source_id) is not among the images of %s"
                             % (source_id, self.path))
        info, anns = self.images[image_id], self.per_image.get(image_id, [])
        xywh = np.asarray([a["bbox"] for a in anns], np.float64).reshape(-1, 4)
        boxes = np.stack([xywh[:, 1], xywh[:, 0], xywh[:, 1] + xywh[:, 3], xywh[:, 0] + xywh[:, 2]], 1)
        return (image_id, (int(info["height"]), int(info["width"])), boxes,
                np.asarray([int(a["category_id"]) - 1 for a in anns], np.int64),
                np.asarray([bool(a.get("iscrowd", 0)) for a in anns], bool),
                np.asarray([float(a["area"]) if "area" in a else float(a["bbox"][2]) * float(a["bbox"][3])
                            for a in anns], np.float64))


def coco_annotations(options, log=None):
    """The CocoAnnotations of options['ann_filename'] when the config names a file that exists; otherwise None —
    groundtruth comes from the records — and one line says so (the reference returns no metrics without the file)."""
    log = log or (lambda msg: print(msg, file=sys.stderr, flush=True))
    path = options["ann_filename"]
    if path and os.path.exists(path):
        return CocoAnnotations(path)
    log("coco_eval_options.eval_ann_filename %s: COCO groundtruth comes from the records (no crowd flags, box areas)"
        % ("is not set" if not path else "%r does not exist" % path))
    return None


def suppress_per_class(boxes, scores, classes, scale, num_classes, nms_type, nms_threshold, sigma, max_per_class,
                       device):
    """The evaluator's per-class NMS of one image (per_image_evaluation.py:233-258, CocoEvaluation :330-357) on the
    device: boxes [n,4] fp32 normalised, scores [n] fp32, classes [n] 0-based; scale multiplies the boxes in double
    (what the evaluator is handed). Invalid boxes are dropped first (_remove_invalid_boxes). -> (boxes [m,4] float64
    scaled, scores [m] fp32, classes [m]) grouped by class."""
    import torch
    from . import ops
    sc = np.broadcast_to(np.asarray(scale, np.float64), (4,))
    bd = np.asarray(boxes, np.float64) * sc
    valid = (bd[:, 0] < bd[:, 2]) & (bd[:, 1] < bd[:, 3])
    classes = np.asarray(classes).astype(np.int64)
    rows = [np.flatnonzero(valid & (classes == c)) for c in range(num_classes)]
    lengths = [len(r) for r in rows]
    order = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if not len(order):
        return np.zeros((0, 4)), np.zeros(0, np.float32), np.zeros(0, np.int64)
    b = torch.from_numpy(np.ascontiguousarray(boxes[order], np.float32)).to(device)
    s = torch.from_numpy(np.ascontiguousarray(scores[order], np.float32)).to(device)
    idx, out_s, cnt = ops.eval_nms(b, s, lengths, nms_type, nms_threshold, sigma, max_per_class,
                                   scale=(float(sc[0]), float(sc[1])))
    idx, out_s, cnt = idx.cpu().numpy(), out_s.cpu().numpy(), cnt.cpu().numpy()
    keep, kept_scores, off = [], [], 0
    for L, k in zip(lengths, cnt):
        keep.append(order[off + idx[off:off + k]])
        kept_scores.append(out_s[off:off + k])
        off += L
    keep = np.concatenate(keep)
    return bd[keep], np.concatenate(kept_scores), classes[keep]


def _raw_records(paths):
    """(source id or file name, encoded image bytes) of every record, in the order the input pipeline delivers them
    (shuffle off, one image per batch): the decoded image and its size, which the resized batch no longer has — the
    submission files and the visualisations are in the frame of the original image (evaluator.py:143, 156-159)."""
    from . import input_reader
    for p in paths:
        for rec in input_reader.read_tfrecord(p):
            f = input_reader.parse_example(rec)
            sid = (f.get("image/source_id") or [b""])[0].decode("utf-8")
            name = (f.get("image/filename") or [b""])[0].decode("utf-8")
            yield sid, name, f.get("image/encoded", [b""])[0]


def _record_subsets(paths):
    """(source id, groundtruth_subset of the record or None when it lacks image/object/subset) of every record, in the
    order the input pipeline delivers them (shuffle off, one image per batch). The field is evaluation-only: no batch
    of the input pipeline carries it, so eval reads it beside the stream, as it reads the original images."""
    from . import input_reader
    for p in paths:
        for rec in input_reader.read_tfrecord(p):
            f = input_reader.parse_example(rec)
            sid = (f.get("image/source_id") or [b""])[0].decode("utf-8")
            yield sid, input_reader.groundtruth_subset(f)


def _download(post, losses):
    """Host copies of one image's postprocess outputs and loss scalars. With losses everything travels in ONE device
    buffer and one copy (float32: the class ids and the count are small integers, exact in it); without, the outputs
    are copied one by one as before."""
    import torch
    if not losses:
        return {k: v.cpu().numpy() for k, v in post.items()}, {}
    keys, names = list(post), list(losses)
    flat = torch.cat([post[k].reshape(-1).to(torch.float32) for k in keys]
                     + [losses[n].reshape(-1) for n in names]).cpu().numpy()
    d, off = {}, 0
    for k in keys:
        n = post[k].numel()
        dtype = torch.empty(0, dtype=post[k].dtype).numpy().dtype
        d[k] = flat[off:off + n].astype(dtype).reshape(tuple(post[k].shape))
        off += n
    vals = {n: float(flat[off + i]) for i, n in enumerate(names)}
    for n, v in vals.items():
        if not np.isfinite(v):                  # evaluator.py:214-216 tf.check_numerics on every term
            raise FloatingPointError("%s is inf or nan." % n)
    return d, vals


def _flags(argv):
    from .train import FLOAT32_MATMUL_PRECISIONS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint_dir", required=True)
    ap.add_argument("--eval_dir", default="")
    ap.add_argument("--pipeline_config_path", required=True)
    ap.add_argument("--eval_training_data", default="false")
    ap.add_argument("--run_once", default="true",
                    help="false: keep evaluating every new state of --checkpoint_dir (eval_config.eval_interval_secs, "
                         "max_evals)")
    ap.add_argument("--logtostderr", action="store_true")
    ap.add_argument("--input_pipeline", choices=("async", "host"), default="async",
                    help="async: decode workers + on-device resize (mtl_ssl_amd.input_pipeline); host: the serial "
                         "generator input_reader.batches (the same images, bit for bit)")
    ap.add_argument("--float32_matmul_precision", choices=FLOAT32_MATMUL_PRECISIONS, default=None,
                    help="how the large fp32 GEMMs multiply, for the whole process (ops.set_float32_matmul_precision; "
                         "see python -m mtl_ssl_amd.train --help). Not given: the process's setting stays")
    return ap.parse_args(sys.argv[1:] if argv is None else argv)


def main(argv=None):
    f = _flags(argv)
    import torch
    import __graft_entry__ as ge
    ge.build()
    from . import checkpoint, config, eval_workflow, evaluation, model_builder, mtl_metrics, ops
    from .train import record_batches, record_paths
    if f.float32_matmul_precision is not None:
        ops.set_float32_matmul_precision(f.float32_matmul_precision)
    cfg = config.parse_pipeline_config(open(f.pipeline_config_path).read())
    ec = cfg.get("eval_config", config.Msg("EvalConfig"))
    use_train = str(f.eval_training_data).lower() in ("1", "true")
    reader = cfg.get("train_input_reader" if use_train else "eval_input_reader", config.Msg())
    K = int(cfg.model.faster_rcnn.num_classes)
    dev = torch.device("cuda", 0)
    model = model_builder.build(cfg.model, False, dev, seed=0)       # built once; every evaluation restores values
    metrics_set = ec.get("metrics_set", "pascal_voc_metrics")
    if isinstance(metrics_set, (list, tuple)):          # the config parser hands a field that may repeat over as a list
        if len(metrics_set) != 1:
            raise ValueError("eval_config.metrics_set: one metric set expected, got %r" % (list(metrics_set),))
        metrics_set = metrics_set[0]
    metrics_set = str(metrics_set)
    coco = "coco" in metrics_set
    limit = int(ec.get("num_examples", 5000))
    rz = cfg.model.faster_rcnn.image_resizer
    nms_type, nms_thr, sigma, iou_thr = eval_nms_options(ec)
    # object_detection_evaluation.py:45-59 / :294-305: per-class caps of the evaluator's NMS
    eval_nms = None if (nms_type == "standard" and nms_thr == 1.0) else (256 if coco else 10000)
    mtl = cfg.model.get("mtl")
    use = {k: mtl is not None and bool(mtl.get(k, False)) for k in ("window", "closeness", "edgemask", "refine")}
    calc_loss = bool(ec.get("calc_loss", False))
    submission = bool(ec.get("submission_format_output", False))
    vis_dir = str(ec.get("visualization_export_dir", "") or "")
    n_vis = int(ec.get("num_visualizations", 10)) if vis_dir else 0
    cats = eval_workflow.categories(K, str(reader.get("label_map_path", "") or "")) if (submission or n_vis) else None
    if submission and not f.eval_dir:
        raise ValueError("eval_config.submission_format_output writes <eval_dir>/detection_results/: give --eval_dir")
    # eval_util.py:489-549: which COCO_Eval/<class>/<metric> keys to report, and the annotation file as groundtruth
    coco_opts = coco_eval_options(ec) if (coco and not submission) else None
    coco_names = coco_class_names(K, str(reader.get("label_map_path", "") or "")) if coco_opts else None
    coco_ann = coco_annotations(coco_opts) if coco_opts else None

    def evaluate_state(fh):
        """One evaluation of the state in the open file fh (eval_util.run_checkpoint_once)."""
        step = checkpoint.load(fh, model.ps)
        if bool(ec.get("use_moving_averages", False)):
            # evaluator.py:330-333: restore variable_averages.variables_to_restore(), i.e. every variable from its
            # `<name>/ExponentialMovingAverage` shadow when the training run kept one
            fh.seek(0)
            n_ema = checkpoint.load_moving_averages(fh, model.ps)
            if n_ema == 0:
                raise ValueError(checkpoint.NO_MOVING_AVERAGES % fh.name)
        model.prepare()
        # evaluator.py:318-322: iou_threshold is PASCAL's matching threshold; COCO keeps its .50:.05:.95
        # the COCO evaluator matches on the device (ops.coco_match): the same numbers as its host loops, bit for bit
        ev = evaluation.CocoDetectionEvaluator(K, device=dev) if coco else evaluation.PascalDetectionEvaluator(K, iou_thr)
        # eval_util.py:300-380: beside it, one PASCAL result per groundtruth subset of the records' image/object/subset,
        # labelled on the device (ops.pascal_match); the legacy keys above stay the host evaluator's
        sub_ev = None if (coco or submission) else evaluation.PascalSubsetEvaluator(K, iou_thr, device=dev)
        subsets = _record_subsets(record_paths(reader)) if sub_ev is not None else None
        any_subsets = False
        mm = mtl_metrics.MtlMetrics()
        missing = {}
        em_counts = []
        closeness_error = None
        loss_sums = {}
        results = []
        images = []
        n_img = 0
        raw = _raw_records(record_paths(reader)) if (submission or n_vis) else None
        stream = record_batches(f.input_pipeline, record_paths(reader), K, 1, (), None, dev, reader,
                                resized_shape=lambda h, w: model.resized_shape(h, w, rz))
        for b in stream:
            if n_img >= limit:
                break
            metrics = not submission
            if calc_loss and metrics:
                # evaluator.py:123-141: calc_loss hands the groundtruth to the is_training=False model
                for key, field, on in (("groundtruth_closeness", "image/object/closeness/text", use["closeness"]),
                                       ("window_boxes", "image/window/...", use["window"]),
                                       ("groundtruth_edgemask", "image/edgemask/masks", use["edgemask"])):
                    if on and b.get(key) is None:
                        raise ValueError("eval_config.calc_loss: the records lack %s, which the loss of this model "
                                         "reads" % field)
                model.provide_groundtruth(b["groundtruth_boxes"], b["groundtruth_classes"],
                                          b["groundtruth_closeness"] if use["closeness"] else None)
                if use["window"]:
                    model.provide_window(b["window_boxes"], b["window_classes"])
                if use["edgemask"]:
                    model.provide_edgemask(b["groundtruth_edgemask"])
            # evaluator.py:123-148: predict -> predict_with_window (the record's groundtruth windows) ->
            # predict_edgemask -> refine -> postprocess; the auxiliary outputs are copied on the device at once (later
            # passes reuse buffers)
            pd = model.predict(model.preprocess(b["images"].to(dev)))
            win = clo = em = None
            if use["window"] and metrics:
                if b.get("window_boxes") is None:
                    missing["mtl/window_map"] = "window boxes / labels (image/window/...)"
                elif len(b["window_boxes"][0]):
                    wb = torch.from_numpy(np.ascontiguousarray(b["window_boxes"][0], np.float32)).to(dev).view(1, -1, 4)
                    win = model.predict_with_window(pd, wb)["window_class_predictions"].clone()
                else:
                    mm.add_window(np.zeros((0, K + 1), np.float32), np.zeros((0, K + 1), np.float32))
            if use["closeness"] and closeness_error is None and metrics:
                if b.get("groundtruth_closeness") is None:
                    missing["mtl/closeness_diff"] = "groundtruth closeness (image/object/closeness/text)"
                else:
                    clo = pd["closeness_predictions"].clone()
            if use["edgemask"] and metrics:
                model.predict_edgemask(pd)
                if b.get("groundtruth_edgemask") is None:
                    missing["mtl/edgemask_ap"] = "groundtruth edge mask (image/edgemask/masks)"
                else:
                    gt_em = b["groundtruth_edgemask"][0]
                    gt0 = torch.from_numpy(np.ascontiguousarray(gt_em[0], np.float32)).to(dev)
                    em = ops.edgemask_agreement(pd["edgemask_predictions"][0].contiguous(), gt0)
                    em_counts.append((em, gt_em.shape[1], gt_em.shape[2]))
            if use["refine"]:
                pd = model.predict_with_mtl_results(pd)
            post = model.postprocess(pd)
            # evaluator.py:211-216: model.loss(prediction_dict) of this image, seeded by its index; the scalars come
            # back with the detections
            losses = model.eval_loss(pd, image_index=n_img) if (calc_loss and metrics) else None
            d, loss_vals = _download(post, losses)
            model.check_device_flags()             # e.g. the refiner's window de-duplication ran out of slots (NaN boxes)
            for k, v in loss_vals.items():
                loss_sums.setdefault(k, []).append(v)
            n = int(d["num_detections"][0])
            H, W = b["images"].shape[1:3]
            if raw is not None:
                sid, name, encoded = next(raw)
                if b.get("source_id") is not None and b["source_id"][0] != sid:
                    raise RuntimeError("record %d: the input pipeline delivered %r, the record file holds %r"
                                       % (n_img, b["source_id"][0], sid))
                image_id = sid or name
                if submission or n_img < n_vis:
                    from .inference import decode_image
                    original = decode_image(encoded)
                    # box_list_ops.to_absolute_coordinates in the original image's frame (evaluator.py:156-159), float32
                    ohw = np.asarray(original.shape[:2] * 2, np.float32)
                    abs_boxes = np.asarray(d["detection_boxes"][0][:n], np.float32) * ohw
                    classes1 = np.asarray(d["detection_classes"][0][:n]).astype(np.int64) + 1    # label_id_offset
                    scores = np.asarray(d["detection_scores"][0][:n], np.float32)
                    if submission:
                        results.append((image_id, abs_boxes, scores, classes1))
                    if n_img < n_vis:
                        gtb = np.asarray(b["groundtruth_boxes"][0], np.float32).reshape(-1, 4) * ohw
                        png = eval_workflow.visualize_detection_results(original, image_id, abs_boxes, scores, classes1,
                                                                        gtb, cats, vis_dir, dev)
                        if png and f.eval_dir:         # eval_util.py:660-669: the drawn image as a summary, too
                            images.append((image_id, png, original.shape[0], original.shape[1]))
            if not metrics:
                n_img += 1
                continue
            if win is not None:
                mm.add_window(win.cpu().numpy(), b["window_classes"][0])
            if clo is not None and closeness_error is None:
                # the reference's absolute fp32 boxes (box_list_ops.scale / to_absolute_coordinates), all padded slots
                hw = np.asarray([H, W, H, W], np.float32)
                try:
                    mm.add_closeness(clo.cpu().numpy(), b["groundtruth_closeness"][0],
                                     np.asarray(b["groundtruth_boxes"][0], np.float32).reshape(-1, 4) * hw,
                                     np.asarray(d["detection_boxes"][0], np.float32) * hw)
                except ValueError as e:        # the reference stops with an IndexError; the other metrics stay valid
                    closeness_error = str(e)
            # evaluator.py:137-150 hands the COCO evaluator absolute boxes, the PASCAL one either (IoU is scale-free)
            scale = np.asarray([H, W, H, W], np.float64) if coco else 1.0
            image_key = n_img
            if coco_ann is not None:
                # groundtruth from the annotation file, keyed by the integer source id, in the pixels of the ORIGINAL
                # image (the file's height / width): the detections are scaled to that frame as well
                sid = None if b.get("source_id") is None else b["source_id"][0]
                image_key, (oh, ow), gt_boxes, gt_cls, gt_crowd, gt_area = coco_ann.image(sid)
                scale = np.asarray([oh, ow, oh, ow], np.float64)
                ev.add_single_ground_truth_image_info(image_key, gt_boxes, gt_cls, is_crowd=gt_crowd, areas=gt_area)
            else:
                gt_boxes = np.asarray(b["groundtruth_boxes"][0], np.float64).reshape(-1, 4) * scale
                gt_cls = np.asarray(b["groundtruth_classes"][0]).argmax(1)
                if coco:
                    ev.add_single_ground_truth_image_info(n_img, gt_boxes, gt_cls)
                else:     # evaluator.py:196-201 -> eval_util.py:332-334: PASCAL's difficult boxes are ignored, not missed
                    diff = b.get("groundtruth_difficult")
                    diff = None if diff is None else np.asarray(diff[0], bool)
                    ev.add_single_ground_truth_image_info(n_img, gt_boxes, gt_cls, is_difficult=diff)
                    sid, names = next(subsets)
                    if b.get("source_id") is not None and b["source_id"][0] != sid:
                        raise RuntimeError("record %d: the input pipeline delivered %r, the record file holds %r"
                                           % (n_img, b["source_id"][0], sid))
                    any_subsets |= names is not None
                    sub_ev.add_single_ground_truth_image_info(n_img, gt_boxes, gt_cls, is_difficult=diff, subsets=names)
            if eval_nms is None:
                dets = (np.asarray(d["detection_boxes"][0][:n], np.float64) * scale, d["detection_scores"][0][:n],
                        d["detection_classes"][0][:n])
            else:
                dets = suppress_per_class(
                    d["detection_boxes"][0][:n], d["detection_scores"][0][:n], d["detection_classes"][0][:n], scale, K,
                    nms_type, nms_thr, sigma, eval_nms, dev)
            ev.add_single_detected_image_info(image_key, *dets)
            if sub_ev is not None:
                sub_ev.add_single_detected_image_info(image_key, *dets)
            n_img += 1
        if hasattr(stream, "close"):
            stream.close()
        if raw is not None:
            raw.close()
        if subsets is not None:
            subsets.close()
        if submission:
            # eval_util.py:783-786, 838-841: no metrics, only the files of the test servers
            paths = eval_workflow.save_detection_results_for_submission(results, cats, f.eval_dir, metrics_set)
            print(json.dumps({"global_step": int(step), "num_images": n_img, "submission_files": paths}))
            return {"global_step": int(step), "num_images": n_img, "submission_files": paths,
                    "detections": [dict(image_id=r[0], boxes=r[1], scores=r[2], classes=r[3]) for r in results]}
        if em_counts:
            counts = torch.cat([c for c, _, _ in em_counts]).cpu().numpy()
            for c, (_, h, w) in zip(counts, em_counts):
                mm.add_edgemask(int(c), h, w)
        res = ev.evaluate()
        out = {"global_step": int(step), "num_images": n_img}
        for k, v in res.items():
            # the per-class curves stay in the evaluator; the per-category COCO table is reported through the
            # COCO_Eval/ keys that coco_eval_options asks for
            if k not in ("precisions", "recalls", "per_class_stats"):
                out[k] = _plain(v)
        if coco_opts is not None:
            out.update(coco_eval_keys(res, coco_opts, coco_names))
        sres = None
        if any_subsets:
            sres = sub_ev.evaluate()
            out.update(pascal_subset_keys(sres, iou_thr, coco_class_names(K, str(reader.get("label_map_path", "") or ""))))
        mres = mm.evaluate()
        if closeness_error is not None:
            mres.pop("mtl/closeness_diff", None)
            warnings.warn("mtl/closeness_diff left out: " + closeness_error)
        for key, field in sorted(missing.items()):
            if key not in mres:
                warnings.warn("%s left out: no evaluated record carries the %s it needs" % (key, field))
        out.update(mres)
        for k, v in loss_sums.items():                       # eval_util.py:877-882 aggregated_loss: the mean over the images
            out["Loss/" + k] = float(np.mean(v))
        print(json.dumps(out), flush=True)
        if f.eval_dir:
            os.makedirs(f.eval_dir, exist_ok=True)
            with open(os.path.join(f.eval_dir, "metrics-%d.json" % step), "w") as fh_out:
                json.dump(out, fh_out)
            eval_workflow.write_eval_summaries(f.eval_dir, out, images, step)
            if sres is not None:        # eval_util.py:186-203: the macro-averaged PR curve of every subset, as text
                evaluation.write_pr_curves(f.eval_dir, sres["precisions"], sres["recalls"], nms_type, nms_thr, sigma)
            # eval_util.py:869-870, 934-997
            eval_workflow.save_best_ckpt(out, fh.name, step, f.eval_dir, metrics_set, str(ec.get("main_subset", "") or ""),
                                         source=fh)
        return out

    if str(f.run_once).lower() in ("1", "true"):
        with open(os.path.join(f.checkpoint_dir, eval_workflow.STATE_NAME), "rb") as fh:
            return evaluate_state(fh)
    # evaluator.py:335-350 -> eval_util.repeated_checkpoint_run
    done = eval_workflow.repeated_checkpoint_run(
        f.checkpoint_dir, evaluate_state, float(ec.get("eval_interval_secs", 120)),
        eval_workflow.max_number_of_evaluations(ec), log=lambda msg: print(msg, file=sys.stderr, flush=True))
    return done[-1]


if __name__ == "__main__":
    main()
