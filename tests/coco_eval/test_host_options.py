"""eval_config.coco_eval_options on the host: the proto defaults, the two ValueErrors, the COCO_Eval/ key names and row
selection, per_class_stats, and the annotation file as groundtruth. The segment tables and the slicing of one match run
into the three maxDets are checked without a GPU through a numpy restatement of the kernel's lane rule
(tests/coco_eval/cases.py simulate_lanes)."""
import json

import numpy as np
import pytest

from mtl_ssl_amd import config
from mtl_ssl_amd import eval as ev_main
from mtl_ssl_amd.evaluation import CocoDetectionEvaluator
from tests.coco_eval import cases


def _eval_config(text):
    return config.parse_pipeline_config("eval_config { metrics_set: 'coco_metrics' %s }" % text).eval_config


def test_defaults_are_the_protos():
    opts = _eval_config("coco_eval_options { }").coco_eval_options
    assert opts.kind == "CocoEvalOptions"
    assert opts.eval_metric_index == [] and opts.eval_class_type == 0
    assert opts.eval_ann_filename == "../data/mscoco/annotations/instances_val2017.json"
    assert ev_main.coco_eval_options(_eval_config("")) is None
    # the default file name is no file the config named: groundtruth stays with the records
    assert ev_main.coco_eval_options(_eval_config("coco_eval_options { }")) == dict(
        metric_index=[0], class_type=0, ann_filename=None)
    got = ev_main.coco_eval_options(_eval_config(
        "coco_eval_options { eval_metric_index: 8 eval_metric_index: 0 eval_metric_index: 1 eval_class_type: 1 "
        "eval_ann_filename: 'a/b.json' }"))
    assert got == dict(metric_index=[0, 1, 8], class_type=1, ann_filename="a/b.json")


@pytest.mark.parametrize("text,what", [("eval_metric_index: 12", "eval_metric_index"),
                                       ("eval_metric_index: 0 eval_metric_index: -1", "eval_metric_index"),
                                       ("eval_class_type: 2", "eval_class_type"),
                                       ("eval_class_type: -1", "eval_class_type")])
def test_out_of_range_options_are_the_references_value_errors(text, what):
    with pytest.raises(ValueError, match="^%s$" % what):
        ev_main.coco_eval_options(_eval_config("coco_eval_options { %s }" % text))


@pytest.fixture(scope="module")
def filled():
    ev = cases.fill_random(CocoDetectionEvaluator(3), 12, seed=2)
    return ev, ev.evaluate()


def test_key_names_and_rows(filled, tmp_path):
    _, res = filled
    assert res["per_class_stats"].shape == (3, 12)
    names = ev_main.coco_class_names(3)
    assert names == {1: "category_1", 2: "category_2", 3: "category_3"}
    keys = ev_main.coco_eval_keys(res, dict(metric_index=[0], class_type=0), names)
    assert keys == {"COCO_Eval/All/AP": res["stats"][0]}
    keys = ev_main.coco_eval_keys(res, dict(metric_index=[0, 1, 8], class_type=1), names)
    assert list(keys) == ["COCO_Eval/%s/%s" % (c, m) for c in ("All", "category_1", "category_2", "category_3")
                          for m in ("AP", "AP_IoU50", "AR_max100")]
    for k in range(3):
        for i, m in ((0, "AP"), (1, "AP_IoU50"), (8, "AR_max100")):
            assert keys["COCO_Eval/category_%d/%s" % (k + 1, m)] == res["per_class_stats"][k, i]
    assert keys["COCO_Eval/All/AR_max100"] == res["AR_100"]
    every = ev_main.coco_eval_keys(res, dict(metric_index=list(range(12)), class_type=0), names)
    assert [k.split("/")[-1] for k in every] == list(ev_main.COCO_METRIC_NAMES) and list(every.values()) == list(res["stats"])
    # a label map names the rows; a category it does not name has none (here id 2)
    path = tmp_path / "map.pbtxt"
    path.write_text("item { id: 1 name: 'cat' }\nitem { id: 3 name: 'dog' }\nitem { id: 7 name: 'beyond num_classes' }\n")
    names = ev_main.coco_class_names(3, str(path))
    assert names == {1: "cat", 3: "dog"}
    keys = ev_main.coco_eval_keys(res, dict(metric_index=[5], class_type=1), names)
    assert keys == {"COCO_Eval/All/AP_large": res["stats"][5], "COCO_Eval/cat/AP_large": res["per_class_stats"][0, 5],
                    "COCO_Eval/dog/AP_large": res["per_class_stats"][2, 5]}


def test_per_class_stats_equal_an_evaluator_fed_one_category(filled):
    ev, res = filled
    assert (res["per_class_stats"][:, 0] == res["per_class_ap"]).all()
    assert len({tuple(r) for r in res["per_class_stats"]}) == 3          # the categories differ
    for k in range(ev.K):
        one = CocoDetectionEvaluator(ev.K)
        for key, (b, c, crowd, a) in ev.gt.items():
            one.add_single_ground_truth_image_info(key, b[c == k], c[c == k], crowd[c == k], a[c == k])
        for key, (b, s, c) in ev.dt.items():
            one.add_single_detected_image_info(key, b[c == k], s[c == k], c[c == k])
        alone = one.evaluate()
        assert (alone["stats"] == res["per_class_stats"][k]).all(), (k, alone["stats"], res["per_class_stats"][k])


class _Simulated(CocoDetectionEvaluator):
    """The device path with the kernel replaced by its numpy restatement."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.device = "simulated"

    def match_on_device(self, keys, timings=None):
        tab = self._segment_tables(keys)
        return (tab,) + cases.simulate_lanes(tab, self.IOU_THRS, self.AREA_RNG)


def test_lane_rule_and_one_run_for_three_max_dets_equal_the_host_path():
    ev = cases.fill_hand_made(_Simulated(3), 70)
    tab = ev._segment_tables(cases.keys_of(ev))
    assert cases.assert_match_equals_host(ev, tab, *cases.simulate_lanes(tab, ev.IOU_THRS, ev.AREA_RNG)) == 13 * 12
    host = cases.fill_random(CocoDetectionEvaluator(4, 30), 40, seed=4, max_gt=8, max_dt=40).evaluate()
    sim = cases.fill_random(_Simulated(4, 30), 40, seed=4, max_gt=8, max_dt=40).evaluate()
    for k in ("stats", "per_class_ap", "per_class_stats"):
        assert (host[k] == sim[k]).all(), k
    assert (host["stats"] > 0).sum() >= 10


def test_a_device_that_is_no_gpu_is_refused():
    with pytest.raises(ValueError, match="no CUDA device"):
        CocoDetectionEvaluator(3, device="cpu")
    assert CocoDetectionEvaluator(3).device is None


def _instances(path):
    images = [dict(id=11, height=100, width=200, file_name="a.jpg"), dict(id=12, height=50, width=60, file_name="b.jpg"),
              dict(id=13, height=80, width=80, file_name="c.jpg")]
    anns = [dict(id=1, image_id=11, category_id=2, bbox=[10, 20, 30, 40], area=700.5, iscrowd=0),
            dict(id=2, image_id=11, category_id=1, bbox=[0, 0, 200, 100], area=15000.0, iscrowd=1),
            dict(id=3, image_id=12, category_id=3, bbox=[5.5, 6.5, 10, 20], area=123.0, iscrowd=0)]
    path.write_text(json.dumps(dict(images=images, annotations=anns,
                                    categories=[dict(id=i, name="c%d" % i) for i in (1, 2, 3)])))
    return str(path)


def test_annotation_file_is_the_groundtruth(tmp_path, capsys):
    path = _instances(tmp_path / "instances.json")
    opts = ev_main.coco_eval_options(_eval_config("coco_eval_options { eval_ann_filename: '%s' }" % path))
    ann = ev_main.coco_annotations(opts)
    assert capsys.readouterr().err == ""
    key, hw, boxes, cls, crowd, area = ann.image("11")
    assert key == 11 and hw == (100, 200)
    assert boxes.tolist() == [[20.0, 10.0, 60.0, 40.0], [0.0, 0.0, 100.0, 200.0]]       # xywh -> ymin, xmin, ymax, xmax
    assert cls.tolist() == [1, 0] and crowd.tolist() == [False, True] and area.tolist() == [700.5, 15000.0]
    key, hw, boxes, cls, crowd, area = ann.image(b"13".decode())                         # an image without annotations
    assert key == 13 and boxes.shape == (0, 4) and cls.shape == crowd.shape == area.shape == (0,)
    # the file's crowd flag and area reach the evaluator: the crowd box is no groundtruth, 700.5 is 'small'
    ev = CocoDetectionEvaluator(3)
    for sid in ("11", "12"):
        key, _, boxes, cls, crowd, area = ann.image(sid)
        ev.add_single_ground_truth_image_info(key, boxes, cls, is_crowd=crowd, areas=area)
        ev.add_single_detected_image_info(key, boxes, np.full(len(boxes), 0.9), cls)
    res = ev.evaluate()
    assert res["per_class_stats"][0, 0] == -1.0                   # category 1 holds only the crowd box
    one = 1.0 / (1.0 + np.spacing(1))                             # COCOeval's precision of one hit: tp / (tp + fp + eps)
    assert res["per_class_stats"][1, 3] == one and res["per_class_stats"][1, 4] == -1.0   # 30 x 40 box, area 700.5
    for bad in ("14", "im0", None):
        with pytest.raises(ValueError, match="is not among the images of"):
            ann.image(bad)


def test_missing_or_unset_annotation_file_falls_back_with_one_line(tmp_path, capsys):
    missing = str(tmp_path / "nowhere.json")
    opts = ev_main.coco_eval_options(_eval_config("coco_eval_options { eval_ann_filename: '%s' }" % missing))
    assert ev_main.coco_annotations(opts) is None
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "does not exist" in err and "groundtruth comes from the records" in err
    assert ev_main.coco_annotations(ev_main.coco_eval_options(_eval_config("coco_eval_options { }"))) is None
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "is not set" in err
