"""The host logic around an evaluation (mtl_ssl_amd/eval_workflow.py): which metric decides the best checkpoint and when
it is replaced, the continuous-evaluation loop on a stub evaluate function, the submission formats and the paint list of
the visualisations. No GPU."""
import json
import os

import numpy as np
import pytest

from mtl_ssl_amd import eval_workflow as W

PASCAL = {"global_step": 7, "num_images": 3, "mean_ap": 0.25, "ap_per_class": [0.5, 0.0], "mean_corloc": 0.75,
          "corloc_per_class": [1.0, 0.5], "mtl/window_map": 0.9, "Loss/first_stage_objectness_loss": 0.3}
COCO = {"global_step": 7, "num_images": 3, "AP": 0.125, "AP50": 0.5, "stats": [0.125, 0.5], "per_class_ap": [0.1]}


def test_main_metric_selection():
    assert W.main_metric(PASCAL, "pascal_voc_metrics", "") == ("mean_ap", 0.25)
    assert W.main_metric(PASCAL, "pascal_voc_metrics", "corloc") == ("mean_corloc", 0.75)
    # keys with '/' never match (eval_util.py:947), neither do the lists
    with pytest.raises(ValueError) as e:
        W.main_metric(PASCAL, "pascal_voc_metrics", "window")
    assert "mean_ap" in str(e.value) and "mean_corloc" in str(e.value) and "window" in str(e.value)
    with pytest.raises(ValueError):
        W.main_metric(PASCAL, "pascal_voc_metrics", "Subset person")
    assert W.main_metric(COCO, "coco_metrics", "ignored for coco") == ("AP", 0.125)
    with pytest.raises(ValueError):
        W.main_metric(PASCAL, "no_such_metrics")


def _state(path, payload):
    tmp = str(path) + ".tmp.npz"
    with open(tmp, "wb") as fh:
        fh.write(payload)
    os.replace(tmp, str(path))                     # the trainer's save: write elsewhere, rename over the name


def test_best_checkpoint_is_replaced_only_by_a_better_metric(tmp_path):
    state = tmp_path / "run" / W.STATE_NAME
    state.parent.mkdir()
    eval_dir = str(tmp_path / "eval")
    best = os.path.join(eval_dir, "best")
    _state(state, b"first")
    assert W.save_best_ckpt(dict(PASCAL, mean_ap=0.25), str(state), 7, eval_dir, "pascal_voc_metrics")
    s = json.load(open(os.path.join(best, "summary.json")))
    assert s["mAP"] == 0.25 and s["global_step"] == 7 and s["main_metric"] == "mean_ap"
    assert s["checkpoint_file"] == str(state) and s["mean_corloc"] == 0.75 and s["mtl/window_map"] == 0.9
    assert s["Loss/first_stage_objectness_loss"] == 0.3 and "ap_per_class" not in s
    assert open(os.path.join(best, W.STATE_NAME), "rb").read() == b"first"
    _state(state, b"worse")
    assert not W.save_best_ckpt(dict(PASCAL, mean_ap=0.2), str(state), 8, eval_dir, "pascal_voc_metrics")
    assert not W.save_best_ckpt(dict(PASCAL, mean_ap=float("nan")), str(state), 8, eval_dir, "pascal_voc_metrics")
    assert open(os.path.join(best, W.STATE_NAME), "rb").read() == b"first"
    assert json.load(open(os.path.join(best, "summary.json")))["global_step"] == 7
    _state(state, b"better")
    with open(state, "rb") as fh:                  # the evaluator hands over the file it read
        _state(state, b"even newer, not evaluated")
        assert W.save_best_ckpt(dict(PASCAL, mean_ap=0.5), str(state), 9, eval_dir, "pascal_voc_metrics", source=fh)
    assert open(os.path.join(best, W.STATE_NAME), "rb").read() == b"better"
    s = json.load(open(os.path.join(best, "summary.json")))
    assert s["mAP"] == 0.5 and s["global_step"] == 9
    assert sorted(os.listdir(best)) == [W.STATE_NAME, "summary.json"]           # no temporary file is left
    # COCO picks AP; main_subset selects another PASCAL key
    assert W.save_best_ckpt(COCO, str(state), 9, str(tmp_path / "coco"), "coco_metrics")
    assert json.load(open(str(tmp_path / "coco" / "best" / "summary.json")))["mAP"] == 0.125
    assert W.save_best_ckpt(PASCAL, str(state), 9, str(tmp_path / "sub"), "pascal_voc_metrics", "corloc")
    assert json.load(open(str(tmp_path / "sub" / "best" / "summary.json")))["mAP"] == 0.75


class _Clock:
    """A clock the loop's sleep advances, with things that happen at given times."""

    def __init__(self, events):
        self.t, self.events, self.slept = 0.0, sorted(events, key=lambda e: e[0]), []

    def now(self):
        return self.t

    def sleep(self, secs):
        assert secs > 0
        self.slept.append(secs)
        self.t += secs
        while self.events and self.events[0][0] <= self.t:
            self.events.pop(0)[1]()


def test_continuous_loop_evaluates_each_new_state_once_in_order(tmp_path):
    state = tmp_path / W.STATE_NAME
    # nothing at t=0; the first state lands at t=12, stays for several rounds, the second lands at t=47
    clock = _Clock([(12.0, lambda: _state(state, b"state 1")), (47.0, lambda: _state(state, b"state 2"))])
    seen, logs = [], []

    def evaluate(fh):
        assert fh.name == str(state)
        seen.append((clock.t, fh.read()))
        clock.t += 3.0                                                         # an evaluation takes time
        return len(seen)

    out = W.repeated_checkpoint_run(str(tmp_path), evaluate, eval_interval_secs=10, max_evals=2, sleep=clock.sleep,
                                    clock=clock.now, log=logs.append)
    assert out == [1, 2]
    assert [p for _, p in seen] == [b"state 1", b"state 2"]
    assert [t for t, _ in seen] == [20.0, 50.0]                                # rounds start every 10 s
    # t=0, 10: no model; t=20: evaluated (3 s), the REST of the interval is slept; t=30, 40: unchanged, not re-evaluated
    assert sum("No model found" in m for m in logs) == 2
    assert sum("already evaluated" in m for m in logs) == 2
    assert clock.slept == [10.0, 10.0, 7.0, 10.0, 10.0]
    assert clock.t == 53.0                                                     # returns right after the last evaluation


def test_continuous_loop_limits():
    assert W.max_number_of_evaluations({"max_evals": 0}) is None
    assert W.max_number_of_evaluations({"max_evals": 3}) == 3
    assert W.max_number_of_evaluations({"max_evals": 3, "ignore_groundtruth": True}) == 1
    with pytest.raises(ValueError):
        W.repeated_checkpoint_run("/nonexistent", lambda fh: None, max_evals=-1)


def test_submission_formats(tmp_path):
    boxes = np.float32([[10.25, 20.5, 110.75, 220.0], [0.0, 1.0, 2.0, 3.5]])
    scores, classes = np.float32([0.987654, 0.0004]), np.int64([2, 1])
    cats = W.categories(2)
    assert cats == [{"id": 1, "name": "category_1"}, {"id": 2, "name": "category_2"}]
    results = [("2008_000001.jpg", boxes, scores, classes), ("im7.png", boxes[:1], scores[:1], classes[:1])]
    paths = W.save_detection_results_for_submission(results, cats, str(tmp_path), "pascal_voc_metrics")
    d = tmp_path / "detection_results"
    assert sorted(os.path.basename(p) for p in paths) == ["comp4_det_test_category_1.txt", "comp4_det_test_category_2.txt"]
    assert open(str(d / "comp4_det_test_category_1.txt")).read() == \
        "%s %f %f %f %f %f\n" % ("2008_000001", scores[1], 1.0, 0.0, 3.5, 2.0)
    assert open(str(d / "comp4_det_test_category_2.txt")).read() == \
        "%s %f %f %f %f %f\n" % ("2008_000001", scores[0], 20.5, 10.25, 220.0, 110.75) + \
        "%s %f %f %f %f %f\n" % ("im7", scores[0], 20.5, 10.25, 220.0, 110.75)
    results = [(139, boxes, scores, classes)]
    (path,) = W.save_detection_results_for_submission(results, cats, str(tmp_path), "coco_metrics")
    text = open(path).read()
    assert text == '[{"image_id":139,"category_id":2,"bbox":[20.5,10.2,199.5,100.5],"score":0.988},' \
                   '{"image_id":139,"category_id":1,"bbox":[1.0,0.0,2.5,2.0],"score":0.000}]'
    assert json.loads(text)[0]["bbox"] == [20.5, 10.2, 199.5, 100.5]
    with pytest.raises(ValueError):
        W.save_detection_results_for_submission(results, cats, str(tmp_path), "open_images_metrics")
    label_map = tmp_path / "map.pbtxt"
    label_map.write_text("item { id: 2 name: 'dog' }\nitem { id: 1 name: 'cat' }\n")
    assert [c["name"] for c in W.categories(3, str(label_map))] == ["cat", "dog", "category_3"]


def test_visualization_paint_list():
    det = np.float32([[10, 10, 50, 60], [0, 0, 20, 20], [5, 5, 9, 9]])
    boxes, colors, labels = W.visualization_boxes(det, [0.9, 0.6, 0.5], [1, 2, 3],
                                                  groundtruth_boxes=np.float32([[0, 0, 100, 100], [1, 1, 3, 3]]))
    # groundtruth underneath, smallest area first; then the detections above 0.5, the best one last
    assert boxes.tolist() == [[1, 1, 3, 3], [0, 0, 100, 100], [0, 0, 20, 20], [10, 10, 50, 60]]
    assert colors.tolist() == [list(W.GROUNDTRUTH_COLOR)] * 2 + [list(W.class_color(2)), list(W.class_color(1))]
    assert [l[2][0] for l in labels] == [2, 1]
    many = np.tile(np.float32([[0, 0, 4, 4]]), (30, 1))
    b, _, _ = W.visualization_boxes(many, np.full(30, 0.99), np.ones(30, int))
    assert len(b) == W.MAX_NUM_PREDICTIONS == 20
    assert len(set(W.CLASS_COLORS)) == len(W.CLASS_COLORS) and W.class_color(len(W.CLASS_COLORS) + 1) == W.CLASS_COLORS[1]
