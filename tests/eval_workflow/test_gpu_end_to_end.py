"""python -m mtl_ssl_amd.eval with the fields around the metrics: calc_loss against the CPU oracle's loss functions on
the device's own eval-mode predictions (staged: identical boxes downstream), determinism, unchanged defaults,
submission files, visualisation export and one continuous run in a child process.

Records are 160x224 synthetic PNG examples written with the project's record writer. Tolerance of the loss terms: 1e-3
relative (README: losses on identical boxes), with the floor the whole-step checks use for terms that are 0 in the
oracle — |got - want| <= 1e-3 * max(|want|, 1e-3).

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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K, H, W = 5, 160, 224
FRCNN, RFCN = "smoke_resnet50_mtl.config", "smoke_rfcn_resnet50_mtl.config"
LOSS_KEYS = ["first_stage_localization_loss", "first_stage_objectness_loss", "second_stage_localization_loss",
             "second_stage_classification_loss", "closeness_classification_loss", "window_class_loss", "edgemask_loss",
             "refined_classification_loss"]          # the training loss_dict of the smoke configs (every head on)
# what the new eval_config fields are when a config does not mention them (protos/eval.proto)
PROTO_DEFAULTS = ('calc_loss: false submission_format_output: false main_subset: "" max_evals: 0 '
                  'eval_interval_secs: 120 num_visualizations: 10 visualization_export_dir: "" ignore_groundtruth: false')


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _write_records(path, num_gt, seed, groundtruth=True):
    """One PNG tf.Example per entry of num_gt (that many boxes, 0 allowed) with the converters' window, closeness and
    edge-mask labels; groundtruth=False: a test-set record, image and names only."""
    from PIL import Image
    from mtl_ssl_amd import input_reader as R
    from mtl_ssl_amd import labels
    rng = np.random.RandomState(seed)
    recs = []
    for i, G in enumerate(num_gt):
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        img = np.clip(np.stack([x / W * 255, y / H * 255, (x + y) / (H + W) * 255], -1)
                      + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        ex = {"image/encoded": buf.getvalue(), "image/format": b"png", "image/filename": "im%d.png" % i,
              "image/source_id": "2008_%06d.png" % i, "image/height": np.array([H]), "image/width": np.array([W])}
        if groundtruth:
            cyx, hw = rng.uniform(0.25, 0.75, (G, 2)), rng.uniform(0.2, 0.5, (G, 2))
            b = np.concatenate([cyx - hw / 2, cyx + hw / 2], 1).clip(0, 1).astype(np.float32).reshape(-1, 4)
            cls = rng.randint(0, K, G)
            abs_b = b * [H, W, H, W]
            if G:
                wb, wl = labels.random_windows(abs_b, cls + 1, W, H, K, rng, 6)
                clo = labels.closeness_labels(abs_b, cls + 1, W, H, K)
            else:            # an image without objects: windows that hold nothing (all background), no closeness rows
                wb = np.float32([[0.1, 0.1, 0.6, 0.5], [0.3, 0.2, 0.9, 0.8]])
                wl = np.zeros((2, K + 1), np.float32)
                wl[:, 0] = 1
                clo = np.zeros((0, K + 1), np.float32)
            em = labels.edgemask(abs_b, W, H).astype(np.float32)
            ex.update({
                "image/object/bbox/ymin": b[:, 0], "image/object/bbox/xmin": b[:, 1],
                "image/object/bbox/ymax": b[:, 2], "image/object/bbox/xmax": b[:, 3],
                "image/object/class/label": (cls + 1).astype(np.int64), "image/object/difficult": np.zeros(G, np.int64),
                "image/window/bbox/ymin": wb[:, 0], "image/window/bbox/xmin": wb[:, 1],
                "image/window/bbox/ymax": wb[:, 2], "image/window/bbox/xmax": wb[:, 3],
                "image/window/labels/text": [" ".join("%.6f" % v for v in row).encode() for row in wl],
                "image/object/closeness/text": [" ".join("%.6f" % v for v in row).encode() for row in clo],
                "image/edgemask/masks": em.reshape(-1), "image/edgemask/height": np.array([em.shape[1]]),
                "image/edgemask/width": np.array([em.shape[2]])})
        recs.append(R.serialize_example(ex))
    R.write_tfrecord(path, recs)
    return recs


def _config(tmp, name, rec, eval_options="", tag="", model_edit=None):
    text = open(os.path.join(ROOT, "configs", name)).read()
    if model_edit is not None:
        assert model_edit[0] in text
        text = text.replace(model_edit[0], model_edit[1], 1)
    text += "\neval_config { num_examples: 10 %s }\n" % eval_options
    text += 'eval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % rec
    p = str(tmp / ("%s%s.config" % (name.split(".")[0], tag)))
    open(p, "w").write(text)
    return p


def _run_dir(tmp, name):
    from tests.inference.test_gpu_end_to_end import _state
    run = tmp / "run"
    run.mkdir(exist_ok=True)
    _state(name, str(run / "model.ckpt.npz"))                  # initial values, global step 3
    return str(run)


def _eval_main(run, cfgp, *more):
    from mtl_ssl_amd import eval as ev
    out = ev.main(["--checkpoint_dir=" + run, "--pipeline_config_path=" + cfgp, "--input_pipeline=host"] + list(more))
    torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------ eval loss, staged parity
def _device_losses(cfgp, run):
    """Per image of the config's records: (batch, host copies of the eval-mode prediction_dict, {loss: float})."""
    from mtl_ssl_amd import checkpoint, config, model_builder
    from mtl_ssl_amd.train import record_batches, record_paths
    cfg = config.parse_pipeline_config(open(cfgp).read())
    dev = torch.device("cuda", 0)
    model = model_builder.build(cfg.model, False, dev, seed=0)
    checkpoint.load(os.path.join(run, "model.ckpt.npz"), model.ps)
    model.prepare()
    rz = cfg.model.faster_rcnn.image_resizer
    out = []
    for i, b in enumerate(record_batches("host", record_paths(cfg.eval_input_reader), K, 1, (), None, dev,
                                         cfg.eval_input_reader,
                                         resized_shape=lambda h, w: model.resized_shape(h, w, rz))):
        model.provide_groundtruth(b["groundtruth_boxes"], b["groundtruth_classes"], b["groundtruth_closeness"])
        model.provide_window(b["window_boxes"], b["window_classes"])
        model.provide_edgemask(b["groundtruth_edgemask"])
        pd = model.predict(model.preprocess(b["images"]))
        wb = torch.from_numpy(np.ascontiguousarray(b["window_boxes"][0])).to(dev).view(1, -1, 4)
        model.predict_with_window(pd, wb)
        model.predict_edgemask(pd)
        pd = model.predict_with_mtl_results(pd)
        grads_before = int(torch.count_nonzero(model.ps.grads))
        losses = model.eval_loss(pd, image_index=i)
        assert "_d" not in pd and int(torch.count_nonzero(model.ps.grads)) == grads_before == 0
        host = {k: v.cpu().numpy() for k, v in pd.items() if torch.is_tensor(v) and not k.startswith("_")}
        host["image_shape"] = pd["image_shape"]
        out.append((b, host, {k: float(v.item()) for k, v in losses.items()}))
    seed = model.seed
    del model
    torch.cuda.empty_cache()
    return cfg, seed, out


def _oracle_losses(cfg, seed, b, pd, index):
    """faster_rcnn_meta_arch.py:1514-1589 with oracle/frcnn_losses.py on the device's prediction arrays."""
    from oracle import frcnn_losses as L
    fr, mtl = cfg.model.faster_rcnn, cfg.model.mtl
    _, h, w, _ = pd["image_shape"]
    hw = np.float32([h, w, h, w])
    gt_abs = np.asarray(b["groundtruth_boxes"][0], np.float32).reshape(-1, 4) * hw
    onehot = np.asarray(b["groundtruth_classes"][0], np.float32).reshape(-1, K)
    cls_bg = np.concatenate([np.zeros((len(onehot), 1), np.float32), onehot], 1)
    clo = np.asarray(b["groundtruth_closeness"][0], np.float32).reshape(-1, K + 1)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(pd[k]))
    want = {}
    tg = L.rpn_targets(pd["anchors"], [gt_abs], int(fr.first_stage_minibatch_size),
                       float(fr.first_stage_positive_balance_fraction), seed, step=index)
    want.update(L.loss_rpn(t("rpn_box_encodings"), t("rpn_objectness_predictions_with_background"), tg,
                           float(fr.first_stage_localization_loss_weight), float(fr.first_stage_objectness_loss_weight)))
    nump = pd["num_proposals"]
    dt = L.detector_targets(pd["proposal_boxes"], [gt_abs], [cls_bg], [clo])
    want.update(L.loss_box_classifier(t("refined_box_encodings"), t("class_predictions_with_background"), nump, dt,
                                      float(fr.second_stage_localization_loss_weight),
                                      float(fr.second_stage_classification_loss_weight),
                                      closeness_predictions=t("closeness_predictions"),
                                      closeness_weight=float(mtl.closeness_loss_weight)))
    want.update(L.loss_refined_classifier(t("mtl_refined_class_predictions_with_background"), nump, dt,
                                          float(mtl.refined_classification_loss_weight)))
    want.update(L.loss_window_class(t("window_class_predictions"), b["window_classes"][0],
                                    float(mtl.window_class_loss_weight)))
    want.update(L.loss_edgemask(t("edgemask_predictions"), np.asarray(b["groundtruth_edgemask"][0])[None],
                                float(mtl.edgemask_loss_weight)))
    return {k: float(v) for k, v in want.items()}


def _check_staged(name, tmp_path, num_gt, model_edit=None):
    from tests import parity_report
    rec = str(tmp_path / "voc.record")
    _write_records(rec, num_gt, 21)
    run = _run_dir(tmp_path, name)
    cfg, seed, outs = _device_losses(_config(tmp_path, name, rec, model_edit=model_edit), run)
    assert len(outs) == len(num_gt)
    worst = 0.0
    for i, (b, pd, got) in enumerate(outs):
        assert len(b["groundtruth_boxes"][0]) == num_gt[i]
        want = _oracle_losses(cfg, seed, b, pd, i)
        assert sorted(got) == sorted(want) == sorted(LOSS_KEYS)
        for k in LOSS_KEYS:
            dist = abs(got[k] - want[k]) / max(abs(want[k]), 1e-3)
            print("%s image %d (%d gt, %d proposals) %s: device %.7g oracle %.7g rel %.2e"
                  % (name, i, num_gt[i], int(pd["num_proposals"][0]), k, got[k], want[k], dist))
            worst = max(worst, dist)
            assert np.isfinite(got[k]) and dist <= 1e-3, (k, i, got[k], want[k])
    parity_report.LINES.append("eval-mode loss %s%s: max rel distance to the oracle %.2e over %d images"
                               % (name, " (few proposals)" if model_edit else "", worst, len(outs)))
    return cfg, outs


def test_eval_loss_matches_oracle_on_device_predictions(tmp_path):
    """Every padded proposal gets a target (no second-stage sample); an image without groundtruth boxes among them."""
    cfg, outs = _check_staged(FRCNN, tmp_path, [2, 0, 3])
    n2 = int(cfg.model.faster_rcnn.first_stage_max_proposals)
    assert all(o[1]["proposal_boxes"].shape == (1, n2, 4) for o in outs)
    zero = outs[1][2]
    assert zero["second_stage_localization_loss"] == 0.0 and zero["closeness_classification_loss"] == 0.0
    assert zero["second_stage_classification_loss"] > 0.0 and zero["first_stage_objectness_loss"] > 0.0


def test_eval_loss_masks_the_padding_when_few_proposals_survive(tmp_path):
    """A strict first-stage NMS leaves fewer than first_stage_max_proposals boxes: the rest are zero-box padding rows,
    masked by the device-side count and left out of the normaliser."""
    edit = ("first_stage_nms_iou_threshold: 0.7", "first_stage_nms_iou_threshold: 0.05")
    cfg, outs = _check_staged(FRCNN, tmp_path, [2, 0], model_edit=edit)
    n2 = int(cfg.model.faster_rcnn.first_stage_max_proposals)
    for _, pd, _ in outs:
        n = int(pd["num_proposals"][0])
        assert 0 < n < n2, "the case does not exercise the padding mask: %d of %d proposals" % (n, n2)
        assert not pd["proposal_boxes"][0, n:].any()


def test_rfcn_eval_loss_matches_oracle(tmp_path):
    _check_staged(RFCN, tmp_path, [2, 0])


# ------------------------------------------------------------------------------ the launcher
def test_calc_loss_reports_every_loss_term_deterministically_and_exports_visualisations(tmp_path):
    from PIL import Image
    rec = str(tmp_path / "voc.record")
    _write_records(rec, [2, 0, 3], 21)
    run = _run_dir(tmp_path, FRCNN)
    vis = str(tmp_path / "vis")
    plain = _eval_main(run, _config(tmp_path, FRCNN, rec, "", "_plain"))
    assert not [k for k in plain if k.startswith("Loss/")]
    opts = 'calc_loss: true num_visualizations: 2 visualization_export_dir: "%s"' % vis
    cfgp = _config(tmp_path, FRCNN, rec, opts, "_loss")
    a = _eval_main(run, cfgp, "--eval_dir=" + str(tmp_path / "eval_a"))
    b = _eval_main(run, cfgp, "--eval_dir=" + str(tmp_path / "eval_b"))
    assert sorted(k for k in a if k.startswith("Loss/")) == sorted("Loss/" + k for k in LOSS_KEYS)
    ja = json.load(open(str(tmp_path / "eval_a" / "metrics-3.json")))
    jb = json.load(open(str(tmp_path / "eval_b" / "metrics-3.json")))
    same = lambda x, y: json.dumps(x, sort_keys=True) == json.dumps(y, sort_keys=True)      # NaN-tolerant ==
    assert same(ja, jb) and same(ja, json.loads(json.dumps(a))) and (ja == jb or "NaN" in json.dumps(ja))
    # calc_loss changes nothing else: every other key as without it
    assert same({k: v for k, v in a.items() if not k.startswith("Loss/")}, plain)
    # the reported value is the mean over the images of the per-image losses (eval_util.py:877-882)
    _, _, outs = _device_losses(cfgp, run)
    for k in LOSS_KEYS:
        assert a["Loss/" + k] == float(np.mean([o[2][k] for o in outs])), k
    # the best checkpoint of a metrics run
    s = json.load(open(str(tmp_path / "eval_a" / "best" / "summary.json")))
    assert s["global_step"] == 3 and s["main_metric"] == "mean_ap" and same(s["mAP"], a["mean_ap"])
    assert open(str(tmp_path / "eval_a" / "best" / "model.ckpt.npz"), "rb").read() == \
        open(os.path.join(run, "model.ckpt.npz"), "rb").read()
    # visualisations: the first num_visualizations images, at the original image size
    assert sorted(os.listdir(vis)) == ["export-2008_000000.png.png", "export-2008_000001.png.png"]
    for p in os.listdir(vis):
        im = Image.open(os.path.join(vis, p))
        assert im.size == (W, H) and im.mode == "RGB"


def test_unset_fields_equal_their_proto_defaults_and_the_detector(tmp_path, monkeypatch):
    """Passes before and after the change: a config that sets none of the new fields gives, byte for byte, the
    metrics file of one that sets them to their proto defaults, and eval's detections are Detector's."""
    from mtl_ssl_amd import eval as ev, inference, model_builder
    rec = str(tmp_path / "voc.record")
    recs = _write_records(rec, [2, 1, 3], 22)
    run = _run_dir(tmp_path, FRCNN)
    captured, real_build = [], model_builder.build

    def build(*a, **kw):
        m = real_build(*a, **kw)
        post = m.postprocess

        def recording(pd):
            d = post(pd)
            captured.append({k: v.cpu().numpy() for k, v in d.items()})
            return d
        m.postprocess = recording
        return m
    monkeypatch.setattr(model_builder, "build", build)
    files = []
    for tag, opts in (("_unset", ""), ("_defaults", PROTO_DEFAULTS)):
        out_dir = str(tmp_path / ("eval" + tag))
        ev.main(["--checkpoint_dir=" + run, "--pipeline_config_path=" + _config(tmp_path, FRCNN, rec, opts, tag),
                 "--eval_dir=" + out_dir])
        files.append(open(os.path.join(out_dir, "metrics-3.json"), "rb").read())
    monkeypatch.setattr(model_builder, "build", real_build)
    assert files[0] == files[1] and b"Loss/" not in files[0]
    assert len(captured) == 2 * len(recs)
    want = [inference.split_outputs(inference.output_tensors(d))[0] for d in captured]
    det = inference.Detector(_config(tmp_path, FRCNN, rec, "", "_det"), os.path.join(run, "model.ckpt"),
                             input_type="tf_example")
    got = [det.detect_examples([r])[0] for r in recs]
    for i, g in enumerate(got + got):
        for k in g:
            assert np.array_equal(g[k], want[i][k]), (i, k)
    del det
    torch.cuda.empty_cache()


@pytest.mark.parametrize("metrics_set", ["pascal_voc_metrics", "coco_metrics"])
def test_submission_files_reproduce_the_reference_formats(metrics_set, tmp_path):
    rec = str(tmp_path / "test.record")
    _write_records(rec, [0, 0], 23, groundtruth=False)          # test-set records: no groundtruth field at all
    run = _run_dir(tmp_path, FRCNN)
    eval_dir = tmp_path / "eval"
    cfgp = _config(tmp_path, FRCNN, rec, 'submission_format_output: true metrics_set: "%s"' % metrics_set)
    out = _eval_main(run, cfgp, "--eval_dir=" + str(eval_dir))
    assert out["num_images"] == 2 and len(out["detections"]) == 2
    assert not [p for p in os.listdir(str(eval_dir)) if p.startswith("metrics-")]
    assert not os.path.exists(str(eval_dir / "best"))
    res = eval_dir / "detection_results"
    dets = out["detections"]
    assert sum(len(d["scores"]) for d in dets) > 0
    for d in dets:             # absolute boxes in the decoded image, 1-based classes
        assert d["boxes"].shape == (len(d["scores"]), 4) and d["boxes"].max() <= max(H, W) and d["boxes"].max() > 1.0
        assert d["classes"].min() >= 1 and d["classes"].max() <= K
    if metrics_set == "coco_metrics":
        assert os.listdir(str(res)) == ["detection_results.json"]
        want = []
        for d in dets:
            for (t, l, b, r), score, c in zip(d["boxes"], d["scores"], d["classes"]):
                bbox = '[%.1f,%.1f,%.1f,%.1f]' % (l, t, r - l, b - t)
                want.append('{"image_id":%s,"category_id":%d,"bbox":%s,"score":%.3f}' % (d["image_id"], c, bbox, score))
        assert open(str(res / "detection_results.json")).read() == "[" + ",".join(want) + "]"
    else:
        names = ["comp4_det_test_category_%d.txt" % c for c in range(1, K + 1)]
        assert sorted(os.listdir(str(res))) == names
        for c in range(1, K + 1):
            want = ""
            for d in dets:
                name = d["image_id"].replace(".jpg", "").replace(".png", "")
                assert name.startswith("2008_") and "." not in name
                for (t, l, b, r), score, cc in zip(d["boxes"], d["scores"], d["classes"]):
                    if cc == c:
                        want += '%s %f %f %f %f %f\n' % (name, score, l, t, r, b)
            assert open(str(res / names[c - 1])).read() == want


def test_continuous_launcher_stops_after_max_evals(tmp_path):
    """The real launcher without --run_once in a child process: one evaluation of the state that is there, then it
    returns by itself (max_evals: 1) long before the interval or the time limit runs out."""
    rec = str(tmp_path / "voc.record")
    _write_records(rec, [2, 1], 24)
    run = _run_dir(tmp_path, FRCNN)
    eval_dir = tmp_path / "eval"
    cfgp = _config(tmp_path, FRCNN, rec, "max_evals: 1 eval_interval_secs: 3600")
    r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.eval", "--checkpoint_dir=" + run, "--run_once=false",
                        "--pipeline_config_path=" + cfgp, "--eval_dir=" + str(eval_dir), "--input_pipeline=host"],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["num_images"] == 2
    assert "Finished evaluation!" in r.stderr
    assert os.path.exists(str(eval_dir / "metrics-3.json")) and os.path.exists(str(eval_dir / "best" / "summary.json"))
