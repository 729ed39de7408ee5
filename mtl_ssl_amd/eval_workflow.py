"""What the evaluator does around the metrics (object_detection/eval_util.py, evaluator.py): the files the PASCAL VOC
and COCO test servers accept (eval_config.submission_format_output), the best-checkpoint copy (main_subset), the loop of
a continuous evaluation (eval_interval_secs, max_evals) and the visualisations (num_visualizations,
visualization_export_dir). Host logic on arrays the launcher already holds; the only device work is the box overlay
(ops.draw_boxes). Nothing here opens the GPU by itself.
"""
import json
import math
import os
import shutil
import time

import numpy as np

STATE_NAME = "model.ckpt.npz"
# eval_util.py:553-562 visualize_detection_results defaults
MIN_SCORE_THRESH = 0.5
MAX_NUM_PREDICTIONS = 20
LINE_THICKNESS = 2                     # utils/visualization_utils.py:387 visualize_boxes_and_labels_on_image_array
GROUNDTRUTH_COLOR = (255, 255, 0)      # boxes without scores are 'yellow' (visualization_utils.py:434-435)
# colour of a detection by its 1-based class id: a fixed table of this project (12 hues x 2 levels, well apart on both
# light and dark images), indexed class_id % len(CLASS_COLORS)
CLASS_COLORS = tuple(
    tuple(int(round(255 * level * c)) for c in rgb)
    for level in (1.0, 0.6)
    for rgb in ((1, 0, 0), (0, 1, 0), (0, 0.4, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 0.5, 0), (0.5, 1, 0),
                (0, 1, 0.5), (0.5, 0, 1), (1, 0, 0.5), (0.6, 0.6, 0.6)))


def class_color(class_id):
    return CLASS_COLORS[int(class_id) % len(CLASS_COLORS)]


# ------------------------------------------------------------------------------ categories
def categories(num_classes, label_map_path=""):
    """[{id, name}] for ids 1..num_classes (utils/label_map_util.py:62-110 convert_label_map_to_categories with
    max_num_classes): the names of input_reader.label_map_path where it names an id, 'category_<id>' otherwise."""
    names = {}
    if label_map_path:
        from .create_pascal_tf_record import read_label_map
        names = {int(i): n for n, i in read_label_map(label_map_path).items()}
    return [{"id": i, "name": names.get(i, "category_%d" % i)} for i in range(1, int(num_classes) + 1)]


# ------------------------------------------------------------------------------ submission files
def pascal_submission_lines(image_id, boxes, scores, classes):
    """eval_util.py:916-928 for one image: [(class id, line)] in detection order. boxes [n,4] absolute
    (ymin, xmin, ymax, xmax) in the decoded image, classes 1-based."""
    name = str(image_id).replace(".jpg", "").replace(".png", "")
    out = []
    for box, score, class_id in zip(boxes, scores, classes):
        t, l, b, r = box
        out.append((int(class_id), "%s %f %f %f %f %f\n" % (name, score, l, t, r, b)))
    return out


def coco_submission_entries(image_id, boxes, scores, classes):
    """eval_util.py:895-907 for one image: the JSON objects as the reference formats them (strings)."""
    out = []
    for box, score, class_id in zip(boxes, scores, classes):
        t, l, b, r = box
        bbox = "[%.1f,%.1f,%.1f,%.1f]" % (l, t, r - l, b - t)
        out.append('{"image_id":%s,"category_id":%d,"bbox":%s,"score":%.3f}' % (image_id, class_id, bbox, score))
    return out


def save_detection_results_for_submission(results, cats, eval_dir, metrics_set):
    """eval_util.py:884-931. results: [(image_id, boxes [n,4] absolute, scores [n], classes [n] 1-based)] in evaluation
    order. Writes <eval_dir>/detection_results/{detection_results.json | comp4_det_test_<name>.txt} and returns the
    paths. Every file is written under a temporary name and renamed."""
    out_dir = os.path.join(eval_dir, "detection_results")
    os.makedirs(out_dir, exist_ok=True)
    paths = []

    def write(path, text):
        tmp = path + ".tmp"
        with open(tmp, "w") as fh:
            fh.write(text)
        os.replace(tmp, path)
        paths.append(path)

    if "coco" in metrics_set:
        entries = [e for r in results for e in coco_submission_entries(*r)]
        write(os.path.join(out_dir, "detection_results.json"), "[" + ",".join(entries) + "]")
    elif metrics_set == "pascal_voc_metrics":
        per_class = {c["id"]: [] for c in cats}
        for r in results:
            for cid, line in pascal_submission_lines(*r):
                if cid not in per_class:
                    raise ValueError("detection of class id %d: the categories hold ids %s" % (cid, sorted(per_class)))
                per_class[cid].append(line)
        for c in cats:
            write(os.path.join(out_dir, "comp4_det_test_%s.txt" % c["name"]), "".join(per_class[c["id"]]))
    else:
        raise ValueError("Metric not found: {}".format(metrics_set))          # evaluator.py:313-314
    return paths


# ------------------------------------------------------------------------------ best checkpoint
PASCAL_ALL_KEY = "mean_ap"             # this build's single PASCAL mAP: the reference's 'Subset all' value
COCO_AP_KEY = "AP"                     # this build's name of COCO_Eval/All/AP


def main_metric(metrics, metrics_set, main_subset=""):
    """eval_util.py:940-961: (key, value) of the metric that decides the best checkpoint. PASCAL: the first key without
    '/' that holds main_subset — a 'Subset <name> mAP@<thr>IOU' key when the records carry groundtruth subsets; with
    an empty main_subset mean_ap, the mAP over every box that is not difficult (the reference's 'Subset all'). COCO:
    COCO_Eval/All/AP, here 'AP'. A main_subset that matches no scalar key is an error (the reference stops on its
    assert)."""
    if "coco" in metrics_set:
        if COCO_AP_KEY not in metrics:
            raise ValueError("coco metrics without %r: %s" % (COCO_AP_KEY, sorted(metrics)))
        return COCO_AP_KEY, float(metrics[COCO_AP_KEY])
    if metrics_set != "pascal_voc_metrics":
        raise ValueError("Metric not found: {}".format(metrics_set))
    scalar = [k for k, v in metrics.items() if "/" not in k and isinstance(v, (int, float, np.floating, np.integer))
              and not isinstance(v, bool) and k not in ("global_step", "num_images")]
    if not main_subset:
        if PASCAL_ALL_KEY not in metrics:
            raise ValueError("pascal metrics without %r: %s" % (PASCAL_ALL_KEY, sorted(metrics)))
        return PASCAL_ALL_KEY, float(metrics[PASCAL_ALL_KEY])
    for k in scalar:
        if main_subset in k:
            return k, float(metrics[k])
    raise ValueError("eval_config.main_subset %r matches no metric; available: %s" % (main_subset, ", ".join(scalar)))


def save_best_ckpt(metrics, state_file, global_step, eval_dir, metrics_set, main_subset="", source=None):
    """eval_util.py:934-997: keeps a copy of the evaluated state under <eval_dir>/best/ while its main metric is not
    below the recorded one (a NaN never replaces; ties replace, as the reference's `<`). summary.json holds
    checkpoint_file, mAP and every scalar metric like the reference's, plus global_step and main_metric (the key mAP was
    read from). The state is copied under a temporary name and renamed before the summary is; returns True when the
    copy was made. source: the open file the state was evaluated from (copied instead of what state_file names now)."""
    key, value = main_metric(metrics, metrics_set, main_subset)
    best = os.path.join(eval_dir, "best")
    summary_path = os.path.join(best, "summary.json")
    if os.path.exists(summary_path):
        with open(summary_path) as fh:
            old = json.load(fh)
        if "mAP" in old and (math.isnan(value) or value < old["mAP"]):
            return False
    os.makedirs(best, exist_ok=True)
    out = {k: float(v) for k, v in metrics.items()
           if isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, bool)}
    out.update(checkpoint_file=os.path.abspath(state_file), mAP=float(value), global_step=int(global_step),
               main_metric=key)
    tmp = os.path.join(best, STATE_NAME + ".tmp")
    if source is None:
        shutil.copyfile(state_file, tmp)
    else:
        source.seek(0)
        with open(tmp, "wb") as fh:
            shutil.copyfileobj(source, fh)
    os.replace(tmp, os.path.join(best, STATE_NAME))
    with open(summary_path + ".tmp", "w") as fh:
        json.dump(out, fh, indent=2, sort_keys=True)
    os.replace(summary_path + ".tmp", summary_path)
    return True


# ------------------------------------------------------------------------------ continuous evaluation
def state_identity(fh):
    """What tells two saved states apart, from an OPEN state file: the trainer writes a state under another name and
    renames it over model.ckpt.npz, so every save is a new inode with its own modification time, the file under that
    name is always a complete one, and a file that is already open stays the state it was whatever is renamed over its
    name afterwards."""
    st = os.fstat(fh.fileno())
    return (st.st_ino, st.st_mtime_ns, st.st_size)


def max_number_of_evaluations(eval_config):
    """evaluator.py:339-342: 1 with ignore_groundtruth, else max_evals, 0 / unset = None (for ever)."""
    if bool(eval_config.get("ignore_groundtruth", False)):
        return 1
    n = int(eval_config.get("max_evals", 0) or 0)
    return n if n > 0 else None


def repeated_checkpoint_run(checkpoint_dir, evaluate, eval_interval_secs=120, max_evals=None, sleep=time.sleep,
                            clock=time.time, log=None):
    """eval_util.py:1000-1120 repeated_checkpoint_run: until max_evals evaluations were made (None: for ever), open
    <checkpoint_dir>/model.ckpt.npz; a state that is new since the last evaluation is evaluated — evaluate(fh) with the
    open binary file, fh.name its path — and then the rest of eval_interval_secs is slept out (also when there was
    nothing new). Returns the list of evaluate()'s results. The state is identified and read through the one open file,
    so a save that lands during an evaluation neither mixes into it nor is skipped: it is evaluated next round."""
    if max_evals is not None and max_evals <= 0:
        raise ValueError("`max_evals` must be either None or a positive number.")
    log = log or (lambda msg: None)
    path = os.path.join(checkpoint_dir, STATE_NAME)
    last, results = None, []
    while True:
        start = clock()
        try:
            fh = open(path, "rb")
        except FileNotFoundError:
            fh = None
        if fh is None:
            log("No model found in %s. Will try again in %d seconds" % (checkpoint_dir, eval_interval_secs))
        else:
            with fh:
                ident = state_identity(fh)
                if ident == last:
                    log("Found already evaluated checkpoint. Will try again in %d seconds" % eval_interval_secs)
                else:
                    last = ident
                    results.append(evaluate(fh))
            if max_evals is not None and len(results) >= max_evals:
                log("Finished evaluation!")
                return results
        left = start + eval_interval_secs - clock()
        if left > 0:
            sleep(left)


# ------------------------------------------------------------------------------ visualisations
def visualization_boxes(detection_boxes, detection_scores, detection_classes, groundtruth_boxes=None,
                        min_score_thresh=MIN_SCORE_THRESH, max_num_predictions=MAX_NUM_PREDICTIONS):
    """eval_util.py:618-654 as a paint list: the groundtruth boxes underneath, in the reference's ascending-area order
    (:629-631), then the detections visualize_boxes_and_labels_on_image_array keeps (visualization_utils.py:425-428) —
    of the first max_num_predictions rows the ones with score > min_score_thresh — painted in reverse, the best-scoring
    last, i.e. on top (the reference paints in the order of a Python 2 dict, which is unspecified). Boxes absolute float (ymin, xmin, ymax, xmax); classes 1-based.
    -> (boxes int32 [n,4] rounded half-open pixel boxes, colors uint8 [n,3], labels [(ymin, xmin, text, rgb)])."""
    boxes, colors, labels = [], [], []
    if groundtruth_boxes is not None and len(groundtruth_boxes):
        g = np.asarray(groundtruth_boxes, np.float64).reshape(-1, 4)
        for i in np.argsort((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]), kind="stable"):
            boxes.append(g[i])
            colors.append(GROUNDTRUTH_COLOR)
    d = np.asarray(detection_boxes, np.float64).reshape(-1, 4)[:max_num_predictions]
    keep = [i for i in range(len(d)) if detection_scores[i] > min_score_thresh]
    for i in reversed(keep):
        rgb = class_color(detection_classes[i])
        boxes.append(d[i])
        colors.append(rgb)
        labels.append((float(d[i][0]), float(d[i][1]), (int(detection_classes[i]), float(detection_scores[i])), rgb))
    b = np.rint(np.asarray(boxes, np.float64).reshape(-1, 4)).astype(np.int32)
    return b, np.asarray(colors, np.uint8).reshape(-1, 3), labels


def draw_labels(image, labels, names):
    """The label text of the detections on the downloaded image, with PIL's built-in default font: '<name>: <score>%'
    (visualization_utils.py: '{}: {}%'.format(class_name, int(100 * score))) on a filled strip above the box's top-left
    corner, or inside it when the box touches the top edge. image uint8 [H,W,3] -> uint8 [H,W,3]."""
    from PIL import Image, ImageDraw, ImageFont
    im = Image.fromarray(np.ascontiguousarray(image))
    draw = ImageDraw.Draw(im)
    font = ImageFont.load_default()
    for ymin, xmin, (cid, score), rgb in labels:
        text = "%s: %d%%" % (names.get(cid, "N/A"), int(100 * score))
        l, t, r, b = draw.textbbox((0, 0), text, font=font)
        w, h = r - l + 4, b - t + 4
        y0 = ymin - h if ymin - h >= 0 else ymin
        draw.rectangle([xmin, y0, xmin + w, y0 + h], fill=tuple(rgb))
        draw.text((xmin + 2 - l, y0 + 2 - t), text, fill=(0, 0, 0), font=font)
    return np.asarray(im)


def visualize_detection_results(image, tag, detection_boxes, detection_scores, detection_classes, groundtruth_boxes,
                                cats, export_dir, device):
    """eval_util.py:553-672 for one image: outlines on the device (mtlssl_draw_boxes), label text on the host, PNG to
    <export_dir>/export-<tag>.png. Without an export_dir nothing is drawn (write_eval_summaries adds the files that were
    drawn to eval_dir's event file). image: uint8 [H,W,3] as decoded. Returns the path or None."""
    if not export_dir:
        return None
    import torch
    from PIL import Image
    from . import ops
    boxes, colors, labels = visualization_boxes(detection_boxes, detection_scores, detection_classes, groundtruth_boxes)
    dev_img = torch.from_numpy(np.ascontiguousarray(image, np.uint8)).to(device)
    ops.draw_boxes(dev_img, torch.from_numpy(boxes).to(device), torch.from_numpy(colors).to(device), LINE_THICKNESS)
    out = draw_labels(dev_img.cpu().numpy(), labels, {c["id"]: c["name"] for c in cats})
    os.makedirs(export_dir, exist_ok=True)
    path = os.path.join(export_dir, "export-{}.png".format(tag))
    Image.fromarray(out).save(path, format="PNG")
    return path


# ------------------------------------------------------------------------------ summaries
def scalar_metrics(metrics):
    """The (key, value) pairs of a metrics dict that are plain numbers, keys sorted (eval_util.py:58-80 write_metrics)."""
    return [(k, float(metrics[k])) for k in sorted(metrics)
            if isinstance(metrics[k], (int, float, np.floating, np.integer)) and not isinstance(metrics[k], bool)]


def write_eval_summaries(eval_dir, metrics, images, global_step):
    """eval_util.py:58-80 and :660-669: one event file in eval_dir per evaluated state, holding a scalar per numeric key
    of `metrics` (Loss/* and mtl/* among them) and an image summary `<tag>/image` per drawn visualisation — images:
    [(tag, path of the PNG visualize_detection_results wrote, height, width)] — all at the state's global step.
    Returns the file's path."""
    from . import summaries
    with summaries.SummaryWriter(eval_dir) as w:
        for k, v in scalar_metrics(metrics):
            w.add_scalar(k, v, global_step)
        for tag, path, height, width in images:
            with open(path, "rb") as fh:
                w.add_image("%s/image" % tag, fh.read(), height, width, global_step)
        return w.path
