"""python -m mtl_ssl_amd.eval end to end on the GPU: records with the converters' window, closeness and edge-mask labels,
3 training steps, then the metrics JSON against a host restatement computed from the same model's device outputs —
the three mtl/* keys, the default options against the evaluator called directly, and soft-Gaussian NMS with matching
at 0.7 against the numpy NMS path. R-FCN once.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage, after every kernel-parity module."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_mtl_metrics import edgemask_labels_numpy, eval_nms_numpy, portable_exp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K, H, W, N_REC = 5, 160, 224, 4
# the closeness metric indexes the per-proposal rows (first_stage_max_proposals: 40) with a detection slot
POST = ("second_stage_post_processing { batch_non_max_suppression { score_threshold: 0.0 iou_threshold: 0.6 "
        "max_detections_per_class: 40 max_total_detections: 40 } score_converter: SOFTMAX }\n")
SOFT = 'nms_type: "soft-gaussian" nms_threshold: 0.5 soft_nms_sigma: 0.5 iou_threshold: 0.7'


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _write_records(path, rng):
    """PNG tf.Examples with the fields create_pascal_tf_record.py writes, labels from mtl_ssl_amd.labels."""
    from PIL import Image
    from mtl_ssl_amd import input_reader as R
    from mtl_ssl_amd import labels
    recs = []
    for i in range(N_REC):
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        img = np.clip(np.stack([x / W * 255, y / H * 255, (x + y) / (H + W) * 255], -1)
                      + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)
        G = int(rng.randint(1, 4))
        cyx, hw = rng.uniform(0.25, 0.75, (G, 2)), rng.uniform(0.2, 0.5, (G, 2))
        b = np.concatenate([cyx - hw / 2, cyx + hw / 2], 1).clip(0, 1).astype(np.float32)
        cls = rng.randint(0, K, G)
        abs_b = b * [H, W, H, W]
        wb, wl = labels.random_windows(abs_b, cls + 1, W, H, K, rng, 6)
        clo = labels.closeness_labels(abs_b, cls + 1, W, H, K)
        em = labels.edgemask(abs_b, W, H).astype(np.float32)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        recs.append(R.serialize_example({
            "image/encoded": buf.getvalue(), "image/format": b"png", "image/filename": "im%d.png" % i,
            "image/source_id": str(i), "image/height": np.array([H]), "image/width": np.array([W]),
            "image/object/bbox/ymin": b[:, 0], "image/object/bbox/xmin": b[:, 1],
            "image/object/bbox/ymax": b[:, 2], "image/object/bbox/xmax": b[:, 3],
            "image/object/class/label": (cls + 1).astype(np.int64), "image/object/difficult": np.zeros(G, np.int64),
            "image/window/bbox/ymin": wb[:, 0], "image/window/bbox/xmin": wb[:, 1],
            "image/window/bbox/ymax": wb[:, 2], "image/window/bbox/xmax": wb[:, 3],
            "image/window/labels/text": [" ".join("%.6f" % v for v in row).encode() for row in wl],
            "image/object/closeness/text": [" ".join("%.6f" % v for v in row).encode() for row in clo],
            "image/edgemask/masks": em.reshape(-1), "image/edgemask/height": np.array([em.shape[1]]),
            "image/edgemask/width": np.array([em.shape[2]])}))
    R.write_tfrecord(path, recs)


def _config(tmp, name, rec, eval_options="", tag=""):
    text = open(os.path.join(ROOT, "configs", name)).read()
    text = text.replace("    num_classes: 5\n", "    num_classes: 5\n    " + POST, 1)
    assert POST in text
    text += '\ntrain_input_reader { tf_record_input_reader { input_path: "%s" } }\n' % rec
    text += "eval_config { num_examples: %d %s }\n" % (N_REC, eval_options)
    text += 'eval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % rec
    p = str(tmp / ("%s%s.config" % (name.split(".")[0], tag)))
    open(p, "w").write(text)
    return p


def _run(args, timeout=900):
    r = subprocess.run([sys.executable, "-m"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _eval(run, cfgp):
    r = _run(["mtl_ssl_amd.eval", "--checkpoint_dir=" + run, "--pipeline_config_path=" + cfgp])
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def _device_outputs(cfgp, run):
    """The evaluator's program, restated: predict -> predict_with_window on the record's windows -> predict_edgemask
    -> refine -> postprocess, one image at a time, everything the metrics read copied to the host."""
    from mtl_ssl_amd import checkpoint, config, model_builder
    from mtl_ssl_amd.train import record_batches, record_paths
    cfg = config.parse_pipeline_config(open(cfgp).read())
    dev = torch.device("cuda", 0)
    model = model_builder.build(cfg.model, False, dev, seed=0)
    checkpoint.load(os.path.join(run, "model.ckpt.npz"), model.ps)
    model.prepare()
    rz = cfg.model.faster_rcnn.image_resizer
    out = []
    for b in record_batches("host", record_paths(cfg.eval_input_reader), K, 1, (), None, dev, cfg.eval_input_reader,
                            resized_shape=lambda h, w: model.resized_shape(h, w, rz)):
        pd = model.predict(model.preprocess(b["images"]))
        wb = torch.from_numpy(np.ascontiguousarray(b["window_boxes"][0])).to(dev).view(1, -1, 4)
        win = model.predict_with_window(pd, wb)["window_class_predictions"].cpu().numpy()
        clo = pd["closeness_predictions"].cpu().numpy()
        em = model.predict_edgemask(pd)["edgemask_predictions"][0].cpu().numpy()
        post = {k: v.cpu().numpy() for k, v in model.postprocess(model.predict_with_mtl_results(pd)).items()}
        out.append(dict(b=b, win=win, clo=clo, em=em, post=post, hw=tuple(b["images"].shape[1:3])))
    del model
    torch.cuda.empty_cache()
    return out


def _pascal(outs, thr, nms=None):
    from mtl_ssl_amd import evaluation
    ev = evaluation.PascalDetectionEvaluator(K, thr)
    changed = False
    for i, o in enumerate(outs):
        b, d = o["b"], o["post"]
        n = int(d["num_detections"][0])
        ev.add_single_ground_truth_image_info(i, np.asarray(b["groundtruth_boxes"][0], np.float64).reshape(-1, 4),
                                              np.asarray(b["groundtruth_classes"][0]).argmax(1),
                                              np.asarray(b["groundtruth_difficult"][0], bool))
        boxes, scores, cls = d["detection_boxes"][0][:n], d["detection_scores"][0][:n], d["detection_classes"][0][:n]
        if nms is not None:          # the numpy path: per class, after _remove_invalid_boxes
            bd = boxes.astype(np.float64)
            valid = (bd[:, 0] < bd[:, 2]) & (bd[:, 1] < bd[:, 3])
            kb, ks, kc = [], [], []
            for c in range(K):
                rows = np.flatnonzero(valid & (cls.astype(int) == c))
                idx, s = eval_nms_numpy(boxes[rows], scores[rows], np.ones(4), *nms, exp=portable_exp)
                kb.append(bd[rows[idx]])
                ks.append(s)
                kc.append(np.full(len(idx), c))
                changed |= not np.array_equal(s, np.sort(scores[rows])[::-1][:len(s)])
            boxes, scores, cls = np.concatenate(kb), np.concatenate(ks), np.concatenate(kc)
        ev.add_single_detected_image_info(i, np.asarray(boxes, np.float64), scores, cls)
    return ev.evaluate(), changed


def _mtl(outs):
    from mtl_ssl_amd import mtl_metrics as M
    win, clo, em = [], [], []
    for o in outs:
        b, (h, w) = o["b"], o["hw"]
        win.append(M.window_image_map(o["win"], b["window_classes"][0]))
        hw = np.float32([h, w, h, w])
        hits = M.closeness_image_hits(o["clo"], b["groundtruth_closeness"][0], M.closeness_slots(
            np.asarray(b["groundtruth_boxes"][0], np.float32) * hw, o["post"]["detection_boxes"][0] * hw))
        if hits:
            clo.append(np.mean(hits))
        gt = b["groundtruth_edgemask"][0][0]
        em.append(np.sum(edgemask_labels_numpy(o["em"], *gt.shape) == gt) / gt.size)
    return {"mtl/window_map": float(np.mean(win)), "mtl/closeness_diff": float(np.mean(clo)) if clo else 0.0,
            "mtl/edgemask_ap": float(np.mean(em))}


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def test_eval_reports_mtl_metrics_and_honours_the_nms_options(tmp_path):
    rec = str(tmp_path / "voc.record")
    _write_records(rec, np.random.RandomState(11))
    name = "smoke_resnet50_mtl.config"
    cfgp = _config(tmp_path, name, rec)
    run = str(tmp_path / "run")
    _run(["mtl_ssl_amd.train", "--train_dir=" + run, "--pipeline_config_path=" + cfgp, "--num_steps=3"])
    out, _ = _eval(run, cfgp)
    assert out["num_images"] == N_REC
    outs = _device_outputs(cfgp, run)
    # the three multi-task metrics equal the host restatement of the same model's device outputs
    want = _mtl(outs)
    assert sorted(k for k in out if k.startswith("mtl/")) == sorted(want)
    for k, v in want.items():
        assert _same(out[k], v), (k, out[k], v)
    assert 0.0 <= out["mtl/edgemask_ap"] <= 1.0
    # default options: the evaluator called directly on the same detections
    res, _ = _pascal(outs, 0.5)
    for k in ("mean_ap", "ap_per_class", "mean_corloc", "corloc_per_class"):
        assert _same(out[k], res[k]), k
    # soft-Gaussian NMS and matching at 0.7: the numpy NMS path
    soft, _ = _eval(run, _config(tmp_path, name, rec, SOFT, "_soft"))
    f32 = lambda v: float(np.float32(v))
    res, changed = _pascal(outs, f32(0.7), ("soft-gaussian", f32(0.5), f32(0.5), 10000))
    assert changed, "soft-NMS rescored nothing: the case does not exercise it"
    for k in ("mean_ap", "ap_per_class", "mean_corloc", "corloc_per_class"):
        assert _same(soft[k], res[k]), (k, soft[k], res[k])
    for k in want:
        assert _same(soft[k], out[k]), k                           # the NMS options leave the MTL metrics alone
    print("default mAP %.6f, soft-gaussian@0.7 mAP %.6f" % (out["mean_ap"], soft["mean_ap"]))


def test_rfcn_eval_reports_mtl_metrics(tmp_path):
    from tests.inference.test_gpu_end_to_end import _state
    rec = str(tmp_path / "voc.record")
    _write_records(rec, np.random.RandomState(12))
    name = "smoke_rfcn_resnet50_mtl.config"
    cfgp = _config(tmp_path, name, rec)
    run = tmp_path / "run"
    run.mkdir()
    _state(name, str(run / "model.ckpt.npz"))          # initial values (R-FCN has no training here)
    out, _ = _eval(str(run), cfgp)
    assert out["num_images"] == N_REC
    outs = _device_outputs(cfgp, str(run))
    want = _mtl(outs)
    for k, v in want.items():
        assert _same(out[k], v), (k, out[k], v)
    res, _ = _pascal(outs, 0.5)
    assert _same(out["mean_ap"], res["mean_ap"]) and _same(out["ap_per_class"], res["ap_per_class"])


def test_labels_missing_from_the_records_leave_their_metric_out_with_a_warning(tmp_path):
    """Records without windows / closeness / edge masks (the inference tests' records): no mtl/* key, one warning per
    missing field, and every detection metric as before."""
    from mtl_ssl_amd import input_reader
    from tests.inference.test_gpu_end_to_end import SHAPES, _pictures, _records, _state
    rec = str(tmp_path / "plain.record")
    input_reader.write_tfrecord(rec, _records(_pictures(SHAPES[:2], 3)))
    name = "smoke_resnet50_mtl.config"
    run = tmp_path / "run"
    run.mkdir()
    _state(name, str(run / "model.ckpt.npz"))
    text = open(os.path.join(ROOT, "configs", name)).read()
    text += "\neval_config { num_examples: 2 }\n"
    text += 'eval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % rec
    cfgp = str(tmp_path / "plain.config")
    open(cfgp, "w").write(text)
    out, err = _eval(str(run), cfgp)
    assert out["num_images"] == 2 and not any(k.startswith("mtl/") for k in out)
    for key in ("mtl/window_map", "mtl/closeness_diff", "mtl/edgemask_ap"):
        assert key + " left out" in err, key
