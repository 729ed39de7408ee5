"""mtl_ssl_amd.eval on six synthetic records that carry image/object/subset (two overlapping subsets, 'all' holding
every box, and a difficult box) and the MobileNet smoke config: the 'Subset <name> mAP@<thr>IOU' keys equal, with
`==`, a HOST PascalSubsetEvaluator fed the same model's detections, recomputed here; 'Subset all' equals mean_ap; the legacy keys
equal those of a run on the same records with the field stripped; the PR-curve text files are written; main_subset
picks the subset key for the best checkpoint.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage, after every kernel-parity module."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.inference.test_gpu_end_to_end import K, SHAPES, _pictures, _png, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = "smoke_mobilenet_v1_mtl.config"
SIZES = SHAPES + [(168, 120)]
LEGACY = ("mean_ap", "ap_per_class", "corloc_per_class", "mean_corloc", "num_images", "global_step")
# the boxes the records draw from: (ymin, xmin, ymax, xmax normalised, subsets)
BOXES = [(0.2, 0.3, 0.7, 0.8, "all|big"), (0.1, 0.1, 0.3, 0.35, "all"), (0.5, 0.05, 0.95, 0.5, "all|big"),
         (0.6, 0.6, 0.8, 0.85, "all")]


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _records(pictures, with_subsets):
    from mtl_ssl_amd import input_reader as R
    recs = []
    for i, img in enumerate(pictures):
        H, W = img.shape[:2]
        rows = [BOXES[(i + j) % len(BOXES)] for j in range(1 + i % 3)]
        col = lambda j: np.asarray([r[j] for r in rows], np.float32)
        ex = {"image/encoded": _png(img), "image/format": b"png", "image/filename": "im%d.png" % i,
              "image/source_id": str(i), "image/height": np.array([H]), "image/width": np.array([W]),
              "image/object/bbox/ymin": col(0), "image/object/bbox/xmin": col(1),
              "image/object/bbox/ymax": col(2), "image/object/bbox/xmax": col(3),
              "image/object/class/label": np.asarray([1 + (i + j) % K for j in range(len(rows))], np.int64),
              "image/object/difficult": np.asarray([int(i == 2 and j == 0) for j in range(len(rows))], np.int64)}
        if with_subsets:
            ex["image/object/subset"] = [r[4].encode() for r in rows]
        recs.append(R.serialize_example(ex))
    return recs


def _config(tmp, rec, tag, options=""):
    text = open(os.path.join(ROOT, "configs", NAME)).read()
    text += "\neval_config { num_examples: %d %s }\n" % (len(SIZES), options)
    text += 'eval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % rec
    p = str(tmp / ("subsets_%s.config" % tag))
    open(p, "w").write(text)
    return p


def _eval(run, cfgp, *more):
    from mtl_ssl_amd import eval as ev
    out = ev.main(["--checkpoint_dir=" + run, "--pipeline_config_path=" + cfgp, "--input_pipeline=host"] + list(more))
    torch.cuda.empty_cache()
    return out


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The two record files, a state, both eval runs, and per image what the evaluated model detects and what the
    evaluator is handed as groundtruth."""
    from mtl_ssl_amd import checkpoint, config, input_reader, model_builder
    from mtl_ssl_amd.train import record_batches, record_paths
    tmp = tmp_path_factory.mktemp("pascal_subsets")
    pictures = _pictures(SIZES, 5)
    tagged, plain = str(tmp / "tagged.record"), str(tmp / "plain.record")
    input_reader.write_tfrecord(tagged, _records(pictures, True))
    input_reader.write_tfrecord(plain, _records(pictures, False))
    run = tmp / "run"
    run.mkdir()
    _state(NAME, str(run / "model.ckpt.npz"))
    eval_dir = str(tmp / "eval")
    out_tagged = _eval(str(run), _config(tmp, tagged, "tagged", 'main_subset: "big"'), "--eval_dir=" + eval_dir)
    out_plain = _eval(str(run), _config(tmp, plain, "plain"))
    cfg = config.parse_pipeline_config(open(_config(tmp, tagged, "collect")).read())
    dev = torch.device("cuda", 0)
    model = model_builder.build(cfg.model, False, dev, seed=0)
    checkpoint.load(str(run / "model.ckpt.npz"), model.ps)
    model.prepare()
    rz, mtl = cfg.model.faster_rcnn.image_resizer, cfg.model.mtl
    images = []
    subsets = [input_reader.decode_example_uint8(r, K)["groundtruth_subset"] for r in input_reader.read_tfrecord(tagged)]
    for i, b in enumerate(record_batches("host", record_paths(cfg.eval_input_reader), K, 1, (), None, dev,
                                         cfg.eval_input_reader, resized_shape=lambda h, w: model.resized_shape(h, w, rz))):
        assert "groundtruth_subset" not in b                       # the batches do not carry the field
        pd = model.predict(model.preprocess(b["images"].to(dev)))
        if mtl.edgemask:
            model.predict_edgemask(pd)
        if mtl.refine:
            pd = model.predict_with_mtl_results(pd)
        d = {k: v.cpu().numpy() for k, v in model.postprocess(pd).items()}
        n = int(d["num_detections"][0])
        images.append((np.asarray(b["groundtruth_boxes"][0], np.float64).reshape(-1, 4),
                       np.asarray(b["groundtruth_classes"][0]).argmax(1), np.asarray(b["groundtruth_difficult"][0], bool),
                       subsets[i], np.asarray(d["detection_boxes"][0][:n], np.float64), d["detection_scores"][0][:n],
                       d["detection_classes"][0][:n]))
    del model
    torch.cuda.empty_cache()
    assert len(images) == len(SIZES) and sum(len(im[4]) for im in images) > 0
    assert any(im[2].any() for im in images) and all("all" in s.split("|") for im in images for s in im[3])
    return out_tagged, out_plain, images, eval_dir


def test_subset_keys_equal_a_host_evaluator(setup):
    from mtl_ssl_amd.evaluation import PascalSubsetEvaluator
    from tests.pascal_subsets import cases
    out, _, images, _ = setup
    want = cases.fill(PascalSubsetEvaluator(K, 0.5), images).evaluate()
    assert want["subset_names"] == ["all", "big"]
    keys = [k for k in out if k.startswith("Subset ")]
    heads = ["Subset all        mAP@0.5IOU", "Subset big        mAP@0.5IOU"]
    assert keys == heads + ["%s/category_%d" % (h, c + 1) for h in heads for c in range(K)]
    for h, name in zip(heads, want["subset_names"]):
        assert _same(out[h], float(want["mean_ap"][name])), (h, out[h], want["mean_ap"][name])
        for c in range(K):
            assert _same(out["%s/category_%d" % (h, c + 1)], float(want["ap_per_class"][name][c])), (h, c)
    assert not np.array_equal(want["num_gt"]["all"], want["num_gt"]["big"])      # the two subsets differ


def test_subset_all_is_mean_ap_and_the_legacy_keys_are_unchanged(setup):
    out, plain, _, _ = setup
    assert _same(out["Subset all        mAP@0.5IOU"], out["mean_ap"])          # 'all' tags every box of the records
    for c in range(K):
        assert _same(out["Subset all        mAP@0.5IOU/category_%d" % (c + 1)], out["ap_per_class"][c]), c
    assert not [k for k in plain if k.startswith("Subset ")]
    for k in LEGACY:
        assert json.dumps(out[k]) == json.dumps(plain[k]), k
    assert set(out) - {k for k in out if k.startswith("Subset ")} == set(plain)


def test_pr_curve_files_and_the_best_checkpoint(setup):
    out, _, _, eval_dir = setup
    names = sorted(f for f in os.listdir(eval_dir) if f.startswith("pr_curve_"))
    assert names == ["pr_curve_all_standard_1.0.txt", "pr_curve_big_standard_1.0.txt"]
    for n in names:
        for line in open(os.path.join(eval_dir, n)):
            p, r = line.rstrip("\n").split("\t")
            assert 0.0 <= float(p) <= 1.0 and 0.0 <= float(r) <= 1.0
    saved = json.load(open(os.path.join(eval_dir, "metrics-3.json")))
    assert [k for k in saved if k.startswith("Subset ")] == [k for k in out if k.startswith("Subset ")]
    best = json.load(open(os.path.join(eval_dir, "best", "summary.json")))
    assert best["main_metric"] == "Subset big        mAP@0.5IOU"
    assert _same(best["mAP"], out["Subset big        mAP@0.5IOU"])
