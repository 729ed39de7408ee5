"""python -m mtl_ssl_amd.eval as a child process with metrics_set 'coco_metrics' on a handful of synthetic records and a
smoke config: without coco_eval_options the JSON holds exactly the keys it held before the options existed, with them
the COCO_Eval/<class>/<metric> keys join, and with an annotation file the groundtruth is the file's. Every value is
compared with `==` against a HOST evaluator (no device) fed the same model's detections, recomputed here.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage, after every kernel-parity module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.inference.test_gpu_end_to_end import K, SHAPES, _pictures, _records, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = "smoke_resnet50_mtl.config"
N_REC = 4
OPTIONS = "coco_eval_options { eval_metric_index: 0 eval_metric_index: 1 eval_metric_index: 8 eval_class_type: 1 %s}"
PARENT_KEYS = {"global_step", "num_images", "stats", "per_class_ap", "AP", "AP50", "AP75", "AP_small", "AP_medium",
               "AP_large", "AR_1", "AR_10", "AR_100", "AR_small", "AR_medium", "AR_large"}


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _config(tmp, rec, options, tag):
    text = open(os.path.join(ROOT, "configs", NAME)).read()
    text += "\neval_config { num_examples: %d metrics_set: 'coco_metrics' %s }\n" % (N_REC, options)
    text += 'eval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % rec
    p = str(tmp / ("coco_%s.config" % tag))
    open(p, "w").write(text)
    return p


def _eval(run, cfgp):
    r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.eval", "--checkpoint_dir=" + run,
                        "--pipeline_config_path=" + cfgp], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """Records, a state, and the detections the evaluated model gives for them: [(normalised boxes, scores, classes,
    (H, W) of the resized image, groundtruth boxes normalised, groundtruth classes)]."""
    from mtl_ssl_amd import checkpoint, config, input_reader, model_builder
    from mtl_ssl_amd.train import record_batches, record_paths
    tmp = tmp_path_factory.mktemp("coco_eval")
    rec = str(tmp / "plain.record")
    input_reader.write_tfrecord(rec, _records(_pictures(SHAPES[:N_REC], 3)))
    run = tmp / "run"
    run.mkdir()
    _state(NAME, str(run / "model.ckpt.npz"))
    cfgp = _config(tmp, rec, "", "plain")
    cfg = config.parse_pipeline_config(open(cfgp).read())
    dev = torch.device("cuda", 0)
    model = model_builder.build(cfg.model, False, dev, seed=0)
    checkpoint.load(str(run / "model.ckpt.npz"), model.ps)
    model.prepare()
    rz, mtl = cfg.model.faster_rcnn.image_resizer, cfg.model.mtl
    dets = []
    for b in record_batches("host", record_paths(cfg.eval_input_reader), K, 1, (), None, dev, cfg.eval_input_reader,
                            resized_shape=lambda h, w: model.resized_shape(h, w, rz)):
        pd = model.predict(model.preprocess(b["images"].to(dev)))
        if mtl.edgemask:
            model.predict_edgemask(pd)
        if mtl.refine:
            pd = model.predict_with_mtl_results(pd)
        d = {k: v.cpu().numpy() for k, v in model.postprocess(pd).items()}
        n = int(d["num_detections"][0])
        dets.append((d["detection_boxes"][0][:n], d["detection_scores"][0][:n], d["detection_classes"][0][:n],
                     tuple(b["images"].shape[1:3]), np.asarray(b["groundtruth_boxes"][0], np.float64).reshape(-1, 4),
                     np.asarray(b["groundtruth_classes"][0]).argmax(1)))
    del model
    torch.cuda.empty_cache()
    assert len(dets) == N_REC and sum(len(d[0]) for d in dets) > 0
    return tmp, rec, str(run), dets


def _host(dets, groundtruth=None):
    """evaluate() of a host evaluator: groundtruth from the records in the resized image's pixels (what eval hands the
    evaluator), or groundtruth(i) -> (key, (H, W), boxes, classes, crowd, areas) from an annotation file."""
    from mtl_ssl_amd.evaluation import CocoDetectionEvaluator
    ev = CocoDetectionEvaluator(K)
    assert ev.device is None
    for i, (boxes, scores, classes, hw, gb, gc) in enumerate(dets):
        if groundtruth is None:
            key, scale = i, np.asarray(hw * 2, np.float64)
            ev.add_single_ground_truth_image_info(key, gb * scale, gc)
        else:
            key, ohw, gboxes, gcls, crowd, areas = groundtruth(i)
            scale = np.asarray(ohw * 2, np.float64)
            ev.add_single_ground_truth_image_info(key, gboxes, gcls, is_crowd=crowd, areas=areas)
        ev.add_single_detected_image_info(key, np.asarray(boxes, np.float64) * scale, scores, classes)
    return ev.evaluate()


def _same_as_parent_keys(out, want):
    assert out["num_images"] == N_REC
    for k in PARENT_KEYS - {"global_step", "num_images"}:
        assert np.array_equal(np.asarray(out[k], np.float64), np.asarray(want[k], np.float64)), (k, out[k], want[k])


def test_without_options_the_line_is_the_parents(setup):
    tmp, rec, run, dets = setup
    out, _ = _eval(run, _config(tmp, rec, "", "plain"))
    assert set(out) == PARENT_KEYS
    _same_as_parent_keys(out, _host(dets))


def test_options_add_the_coco_eval_keys(setup):
    tmp, rec, run, dets = setup
    out, err = _eval(run, _config(tmp, rec, OPTIONS % "", "options"))
    want = _host(dets)
    _same_as_parent_keys(out, want)
    rows = ["All"] + ["category_%d" % (k + 1) for k in range(K)]
    added = ["COCO_Eval/%s/%s" % (r, m) for r in rows for m in ("AP", "AP_IoU50", "AR_max100")]
    assert set(out) == PARENT_KEYS | set(added)
    assert [k for k in out if k.startswith("COCO_Eval/")] == added            # 'All' first, categories by id
    for i, m in ((0, "AP"), (1, "AP_IoU50"), (8, "AR_max100")):
        assert out["COCO_Eval/All/" + m] == want["stats"][i]
        for k in range(K):
            assert out["COCO_Eval/category_%d/%s" % (k + 1, m)] == want["per_class_stats"][k, i], (k, m)
    assert err.count("groundtruth comes from the records") == 1               # no annotation file was named


def test_annotation_file_replaces_the_records_groundtruth(setup):
    """Groundtruth from an instances JSON keyed by image/source_id, in the original image's pixels: one box of the
    records becomes a crowd box, another gets a segmentation area in the 'small' range."""
    from mtl_ssl_amd.eval import CocoAnnotations
    tmp, rec, run, dets = setup
    images, anns = [], []
    for i, (H, W) in enumerate(SHAPES[:N_REC]):
        images.append(dict(id=i, height=H, width=W, file_name="im%d.png" % i))
        x, y, w, h = 0.3 * W, 0.2 * H, 0.5 * W, 0.5 * H                      # the records' one box
        anns.append(dict(id=i + 1, image_id=i, category_id=1 + i % K, bbox=[x, y, w, h], iscrowd=int(i == 1),
                         area=500.0 if i == 2 else w * h))
    path = str(tmp / "instances.json")
    json.dump(dict(images=images + [dict(id=99, height=10, width=10, file_name="unused.png")], annotations=anns,
                   categories=[dict(id=k + 1, name="c%d" % (k + 1)) for k in range(K)]), open(path, "w"))
    out, err = _eval(run, _config(tmp, rec, OPTIONS % ("eval_ann_filename: '%s' " % path), "ann"))
    ann = CocoAnnotations(path)
    want = _host(dets, lambda i: ann.image(str(i)))
    _same_as_parent_keys(out, want)
    for i, m in ((0, "AP"), (1, "AP_IoU50"), (8, "AR_max100")):
        assert out["COCO_Eval/All/" + m] == want["stats"][i]
        for k in range(K):
            assert out["COCO_Eval/category_%d/%s" % (k + 1, m)] == want["per_class_stats"][k, i], (k, m)
    assert out["COCO_Eval/category_2/AP"] == -1.0                             # its only box is crowd in the file
    assert "groundtruth comes from the records" not in err
