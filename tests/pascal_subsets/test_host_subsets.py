"""Groundtruth subsets on the host: PascalSubsetEvaluator against the reference class's recorded results
(tests/golden/pascal_subset_golden.npz) and against its definition — one PascalDetectionEvaluator run per subset with
is_difficult = ~member — the converter's --subsets flag and the decoder's groundtruth_subset, the metric keys, the
best-checkpoint key and the macro-averaged PR curve (hand-derived answers: the reference's file cannot be run)."""
import io
import os
import re
import warnings

import numpy as np
import pytest

from tests.pascal_subsets import cases


@pytest.fixture(scope="module")
def golden_run():
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    images, z = cases.golden()
    ev = cases.fill(PascalSubsetEvaluator(int(z["num_classes"]), float(z["iou_threshold"])), images)
    assert ev.device is None
    return images, z, ev.evaluate()


def test_golden_set_is_what_the_docstring_promises(golden_run):
    images, z, _ = golden_run
    assert len(images) == 40 and len(z["subset_names"]) == 3 and int(z["num_classes"]) == 3
    assert len(images[3][0]) == 0 and len(images[5][4]) == 0
    assert "" in z["gt_subset"] and any("|" in s for s in z["gt_subset"]) and z["gt_difficult"].any()
    assert len(np.unique(z["dt_scores"])) == len(z["dt_scores"])


def test_equals_the_reference_class(golden_run):
    _, z, res = golden_run
    names = [str(n) for n in z["subset_names"]]
    assert res["subset_names"] == names
    for j, n in enumerate(names):
        assert np.array_equal(res["ap_per_class"][n], z["ap"][j], equal_nan=True), n
        assert res["mean_ap"][n] == z["mean_ap"][j], n
        assert np.array_equal(res["num_gt"][n], z["num_gt"][j]), n
    assert np.array_equal(res["corloc_per_class"], z["corloc"], equal_nan=True)
    assert res["mean_corloc"] == float(z["mean_corloc"])
    assert (z["ap"] > 0).sum() >= 6                              # the set exercises the metric


def test_equals_one_pascal_run_per_subset(golden_run):
    images, z, res = golden_run
    runs = cases.one_run_per_subset(images, res["subset_names"], int(z["num_classes"]))
    for n, (want, num_gt) in runs.items():
        assert np.array_equal(res["ap_per_class"][n], want["ap_per_class"], equal_nan=True)
        assert res["mean_ap"][n] == want["mean_ap"]
        assert np.array_equal(res["num_gt"][n], num_gt)
        assert len(res["precisions"][n]) == len(want["precisions"])
        for a, b in zip(res["precisions"][n] + res["recalls"][n], want["precisions"] + want["recalls"]):
            assert np.array_equal(a, b)
        assert np.array_equal(res["corloc_per_class"], want["corloc_per_class"], equal_nan=True)
        assert res["mean_corloc"] == want["mean_corloc"]


def test_one_subset_of_the_not_difficult_boxes_is_the_existing_evaluator(golden_run):
    from mtl_ssl_amd.evaluation import PascalDetectionEvaluator, PascalSubsetEvaluator
    images = golden_run[0]
    old, new = PascalDetectionEvaluator(3), PascalSubsetEvaluator(3)
    for i, (gb, gc, gd, _, db, ds, dc) in enumerate(images):
        old.add_single_ground_truth_image_info(i, gb, gc, is_difficult=gd)
        old.add_single_detected_image_info(i, db, ds, dc)
        new.add_single_ground_truth_image_info(i, gb, gc, is_difficult=gd, subsets=["all"] * len(gb))
        new.add_single_detected_image_info(i, db, ds, dc)
    want, got = old.evaluate(), new.evaluate()
    assert got["subset_names"] == ["all"]
    assert np.array_equal(got["ap_per_class"]["all"], want["ap_per_class"], equal_nan=True)
    assert got["mean_ap"]["all"] == want["mean_ap"] and got["mean_corloc"] == want["mean_corloc"]
    assert np.array_equal(got["num_gt"]["all"], old.num_gt)


def test_length_mismatch_and_missing_subsets_name_the_image():
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    ev = PascalSubsetEvaluator(2)
    with pytest.raises(ValueError, match="image 'im7': 1 subset strings for 2 groundtruth boxes"):
        ev.add_single_ground_truth_image_info("im7", [[0, 0, 1, 1], [0, 0, 2, 2]], [0, 1], subsets=["a"])
    ev.add_single_ground_truth_image_info("im1", [[0, 0, 1, 1]], [0], subsets=["a"])
    ev.add_single_ground_truth_image_info("im2", [[0, 0, 1, 1]], [0])
    with pytest.raises(ValueError, match="image 'im2' has no groundtruth subsets"):
        ev.evaluate()


def test_all_empty_strings_give_no_subsets_and_a_warning():
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    ev = PascalSubsetEvaluator(2)
    ev.add_single_ground_truth_image_info(0, [[0, 0, 1, 1], [0, 0, 2, 2]], [0, 1], subsets=["", ""])
    ev.add_single_detected_image_info(0, [[0, 0, 1, 1]], [0.5], [0])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = ev.evaluate()
    assert len([w for w in seen if "no groundtruth box names a subset" in str(w.message)]) == 1
    assert res["subset_names"] == [] and res["mean_ap"] == {} and res["ap_per_class"] == {} and res["num_gt"] == {}
    assert res["corloc_per_class"].tolist() == [1.0, 0.0]


def test_a_difficult_box_belongs_to_no_subset():
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    ev = PascalSubsetEvaluator(1)
    ev.add_single_ground_truth_image_info(0, [[0, 0, 2, 2], [5, 5, 7, 7]], [0, 0], is_difficult=[True, False],
                                          subsets=["a", "a"])
    ev.add_single_detected_image_info(0, [[0, 0, 2, 2], [5, 5, 7, 7]], [0.9, 0.8], [0, 0])
    res = ev.evaluate()
    assert res["num_gt"]["a"].tolist() == [1] and res["precisions"]["a"][0].tolist() == [1.0]    # the first is dropped


# ------------------------------------------------------------------------------ records
def _jpeg(W, H):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.full((H, W, 3), 128, np.uint8)).save(buf, format="JPEG")
    return buf.getvalue()


def _annotation():
    box = lambda name, xmin, ymin, xmax, ymax, difficult=0: dict(
        name=name, difficult=difficult, truncated=0, pose="Unspecified", xmin=float(xmin), ymin=float(ymin),
        xmax=float(xmax), ymax=float(ymax))
    # areas 100, 99, 400, 2500
    return dict(folder="VOC2007", filename="a.jpg", width=100, height=80,
                objects=[box("cat", 10, 10, 20, 20), box("dog", 10, 10, 21, 19), box("cat", 0, 0, 20, 20, 1),
                         box("dog", 30, 20, 80, 70)])


def _example(subsets):
    from mtl_ssl_amd import create_pascal_tf_record as C
    from mtl_ssl_amd import labels
    return C.example_from_annotation(_annotation(), _jpeg(100, 80), {"cat": 1, "dog": 2}, 2, labels.PyRandom(0),
                                     num_windows=4, subsets=subsets)


def test_converter_round_trip_and_range_edges():
    from mtl_ssl_amd import create_pascal_tf_record as C
    from mtl_ssl_amd import input_reader
    table = C.parse_subsets("all:0:inf,small:0:100,mid:100:400,large:400:inf")
    assert table == [("all", 0.0, float("inf")), ("small", 0.0, 100.0), ("mid", 100.0, 400.0), ("large", 400.0, float("inf"))]
    ex = input_reader.decode_example_uint8(_example(table), 2)
    # lo <= area < hi: 100 is mid, not small; 99 is small; 400 is large, not mid
    assert ex["groundtruth_subset"] == ["all|mid", "all|small", "all|large", "all|large"]
    assert len(ex["groundtruth_subset"]) == len(ex["groundtruth_boxes"])
    none = input_reader.decode_example_uint8(_example(C.parse_subsets("tiny:0:5")), 2)
    assert none["groundtruth_subset"] == ["", "", "", ""]
    assert C.parse_subsets("all:0:inf") == [("all", 0.0, float("inf"))]            # the reference's table


def test_without_the_flag_the_record_is_unchanged_and_has_no_field():
    from mtl_ssl_amd import input_reader
    plain = _example(None)
    assert "image/object/subset" not in input_reader.parse_example(plain)
    assert "groundtruth_subset" not in input_reader.decode_example_uint8(plain, 2)
    tagged = input_reader.parse_example(_example([("all", 0.0, float("inf"))]))
    tagged.pop("image/object/subset")
    assert input_reader.serialize_example(tagged) == plain                  # the other fields, byte for byte
    # the field does not reach a batch: training, the augmentation programs and the stream state never see it
    ex = input_reader.decode_example(_example([("all", 0.0, float("inf"))]), 2)
    assert "groundtruth_subset" not in input_reader.collate_labels([ex])


@pytest.mark.parametrize("flag, entry", [("all", "all"), ("all:0", "all:0"), ("a:0:1,b:1", "b:1"), (":0:1", ":0:1"),
                                         ("a|b:0:1", "a|b:0:1"), ("a:5:1", "a:5:1"), ("a:x:1", "a:x:1"),
                                         ("a:0:1,,b:1:2", "")])
def test_malformed_subsets_flag_names_the_entry(flag, entry, capsys):
    from mtl_ssl_amd import create_pascal_tf_record as C
    with pytest.raises(ValueError, match=re.escape("--subsets entry %r" % entry)):
        C.parse_subsets(flag)
    with pytest.raises(SystemExit):
        C.main(["--data_dir=/nonexistent", "--output_path=/nonexistent/out.record", "--subsets=" + flag])
    assert ("--subsets entry %r" % entry) in capsys.readouterr().err


def test_command_line_writes_the_field(tmp_path):
    from mtl_ssl_amd import create_pascal_tf_record as C
    from mtl_ssl_amd import input_reader
    root = tmp_path / "VOC2007"
    for d in ("JPEGImages", "Annotations", "ImageSets/Main"):
        (root / d).mkdir(parents=True)
    (root / "JPEGImages" / "a.jpg").write_bytes(_jpeg(100, 80))
    objs = "".join("<object><name>%s</name><difficult>0</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax>"
                   "<ymax>%d</ymax></bndbox></object>" % o for o in (("cat", 10, 10, 20, 20), ("dog", 30, 20, 80, 70)))
    (root / "Annotations" / "a.xml").write_text(
        "<annotation><folder>VOC2007</folder><filename>a.jpg</filename><size><width>100</width><height>80</height>"
        "</size>%s</annotation>" % objs)
    (root / "ImageSets" / "Main" / "aeroplane_train.txt").write_text("a 1\n")
    paths = {}
    for tag, extra in (("plain", []), ("tagged", ["--subsets=all:0:inf,small:0:400"])):
        paths[tag] = str(tmp_path / (tag + ".record"))
        assert C.main(["--data_dir=" + str(tmp_path), "--output_path=" + paths[tag]] + extra) == 1
    (rec,) = input_reader.read_tfrecord(paths["tagged"])
    assert input_reader.decode_example_uint8(rec, 20)["groundtruth_subset"] == ["all|small", "all"]
    (plain,) = input_reader.read_tfrecord(paths["plain"])
    assert "image/object/subset" not in input_reader.parse_example(plain)


# ------------------------------------------------------------------------------ keys and the best checkpoint
def _result():
    return dict(subset_names=["all", "small"], mean_ap={"all": 0.5, "small": float("nan")},
                ap_per_class={"all": np.asarray([0.25, 0.75]), "small": np.asarray([np.nan, np.nan])})


def test_metric_keys_are_the_references():
    from mtl_ssl_amd.eval import coco_class_names, pascal_subset_keys
    keys = pascal_subset_keys(_result(), 0.5, coco_class_names(2))
    assert list(keys) == ["Subset all        mAP@0.5IOU", "Subset small      mAP@0.5IOU",
                          "Subset all        mAP@0.5IOU/category_1", "Subset all        mAP@0.5IOU/category_2",
                          "Subset small      mAP@0.5IOU/category_1", "Subset small      mAP@0.5IOU/category_2"]
    assert keys["Subset all        mAP@0.5IOU"] == 0.5 and keys["Subset all        mAP@0.5IOU/category_2"] == 0.75
    assert np.isnan(keys["Subset small      mAP@0.5IOU"])
    named = pascal_subset_keys(_result(), float(np.float32(0.7)), {2: "dog"})      # a map that names one category
    assert list(named) == ["Subset all        mAP@0.699999988079071IOU", "Subset small      mAP@0.699999988079071IOU",
                           "Subset all        mAP@0.699999988079071IOU/dog", "Subset small      mAP@0.699999988079071IOU/dog"]
    long = pascal_subset_keys(dict(subset_names=["extra_large_x"], mean_ap={"extra_large_x": 1.0},
                                   ap_per_class={"extra_large_x": np.ones(1)}), 0.5, {})
    assert list(long) == ["Subset extra_large_x mAP@0.5IOU"]


def test_main_subset_finds_the_subset_key():
    from mtl_ssl_amd.eval import coco_class_names, pascal_subset_keys
    from mtl_ssl_amd.eval_workflow import main_metric
    metrics = {"global_step": 3, "num_images": 6, "mean_ap": 0.4, "mean_corloc": 0.6}
    metrics.update(pascal_subset_keys(_result(), 0.5, coco_class_names(2)))
    key, value = main_metric(metrics, "pascal_voc_metrics", main_subset="small")
    assert key == "Subset small      mAP@0.5IOU" and np.isnan(value)
    assert main_metric(metrics, "pascal_voc_metrics", main_subset="Subset all")[0] == "Subset all        mAP@0.5IOU"
    assert main_metric(metrics, "pascal_voc_metrics") == ("mean_ap", 0.4)           # empty main_subset: as before


# ------------------------------------------------------------------------------ PR curve (hand-derived)
def test_macro_pr_curve_known_answers():
    from mtl_ssl_amd.evaluation import macro_pr_curve
    a_p, a_r = np.asarray([1.0, 0.5, 0.75, 0.5]), np.asarray([0.5, 0.5, 1.0, 1.0])
    # duplicate recalls keep their highest precision: (0.5, 1.0), (1.0, 0.75); thresholds descend
    assert macro_pr_curve([a_p], [a_r]) == ([0.75, 1.0], [1.0, 0.5])
    b_p, b_r = np.asarray([0.5, 0.25, 0.5]), np.asarray([0.25, 0.25, 0.5])
    # class b never reaches recall 1.0 and adds 0 there; a one-point class and a class without a curve are skipped
    p, r = macro_pr_curve([a_p, None, b_p, np.asarray([1.0])], [a_r, None, b_r, np.asarray([1.0])])
    assert (p, r) == ([0.375, 0.75, 0.75], [1.0, 0.5, 0.25])
    # the precision becomes its running maximum from the high-recall end
    assert macro_pr_curve([np.asarray([0.5, 1.0])], [np.asarray([0.5, 1.0])]) == ([1.0, 1.0], [1.0, 0.5])
    assert macro_pr_curve([], []) == ([], [])
    assert macro_pr_curve([None, np.asarray([1.0])], [None, np.asarray([0.5])]) == ([], [])
    with pytest.raises(ValueError):
        macro_pr_curve([a_p], [])


def test_pr_curve_files(tmp_path):
    from mtl_ssl_amd.evaluation import nms_string, write_pr_curves
    assert nms_string("standard", 1.0, 0.5) == "standard_1.0" and nms_string("soft-gaussian", 0.3, 0.5) == "soft-gaussian_0.5"
    assert nms_string("soft-linear", 0.5, 0.25) == "soft-linear_0.5"
    with pytest.raises(ValueError):
        nms_string("other", 1.0, 0.5)
    curves = {"all": [np.asarray([1.0, 0.5, 0.75, 0.5])], "small": []}
    recalls = {"all": [np.asarray([0.5, 0.5, 1.0, 1.0])], "small": []}
    paths = write_pr_curves(str(tmp_path), curves, recalls, "standard", 1.0, 0.5)
    assert [os.path.basename(p) for p in paths] == ["pr_curve_all_standard_1.0.txt", "pr_curve_small_standard_1.0.txt"]
    assert open(paths[0]).read() == "0.750000\t1.000000\n1.000000\t0.500000\n" and open(paths[1]).read() == ""
