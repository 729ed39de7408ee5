"""Detector and export_inference_graph on the GPU: detections bit for bit equal to what eval.py computes for the same
records, exports (plain and moving averages) that give the source checkpoint's detections, the three input types, and
mixed-size lists against one-at-a-time calls.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage, after every kernel-parity module."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K = 5
SHAPES = [(160, 224), (224, 160), (150, 210), (200, 150), (120, 168)]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _pictures(shapes, seed):
    """Smooth colour ramps with noise: every picture gives the detector something other than flat grey."""
    rng = np.random.RandomState(seed)
    out = []
    for H, W in shapes:
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        base = np.stack([x / W * 255, y / H * 255, (x + y) / (H + W) * 255], -1)
        out.append(np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8))
    return out


def _png(img):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    return buf.getvalue()


def _records(pictures):
    """Lossless (PNG) tf.Examples with one groundtruth box each, what eval_input_reader reads."""
    from mtl_ssl_amd import input_reader as R
    recs = []
    for i, img in enumerate(pictures):
        H, W = img.shape[:2]
        recs.append(R.serialize_example({
            "image/encoded": _png(img), "image/format": b"png", "image/filename": "im%d.png" % i,
            "image/source_id": str(i), "image/height": np.array([H]), "image/width": np.array([W]),
            "image/object/bbox/ymin": np.array([0.2], np.float32), "image/object/bbox/xmin": np.array([0.3], np.float32),
            "image/object/bbox/ymax": np.array([0.7], np.float32), "image/object/bbox/xmax": np.array([0.8], np.float32),
            "image/object/class/label": np.array([1 + i % K], np.int64), "image/object/difficult": np.zeros(1, np.int64)}))
    return recs


def _state(config_name, path):
    """A training state as checkpoint.save writes it: initial values, momentum slots, moving-average shadows (the
    initialiser under another seed, so every shadow differs from its variable), a global step."""
    from mtl_ssl_amd import config, model_builder, params
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", config_name)).read())
    out = {}
    for s in model_builder.variable_specs(cfg.model, is_training=False):
        out[s.name] = params.init_value(s, 1)
        out[s.name + "/Momentum"] = np.zeros(s.shape, np.float32)
        out[s.name + "/ExponentialMovingAverage"] = params.init_value(s, 2)
    out["global_step"] = np.asarray(3, np.int64)
    np.savez(path, **out)
    return path


def _pipeline(tmp, config_name, ema, record=None, n=0):
    text = open(os.path.join(ROOT, "configs", config_name)).read()
    text += "\neval_config { num_examples: %d%s }\n" % (max(n, 1), " use_moving_averages: true" if ema else "")
    if record:
        text += 'eval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % record
    p = str(tmp / ("%s_%s.config" % (config_name.split(".")[0], "ema" if ema else "plain")))
    open(p, "w").write(text)
    return p


def _assert_same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y), what
        for k in x:
            assert x[k].dtype == y[k].dtype == np.float32 and np.array_equal(x[k], y[k]), (what, i, k)


def _untouched(det):
    """No step counter moved, no gradient written."""
    assert det.model.step == 0
    assert int(torch.count_nonzero(det.model.ps.grads)) == 0


@pytest.mark.parametrize("config_name", ["smoke_resnet50_mtl.config", "smoke_mobilenet_v1_mtl.config"])
def test_detector_equals_eval_bit_for_bit(config_name, tmp_path, monkeypatch):
    """eval.py's own loop (async record feed, B=1) with its postprocess outputs captured, against Detector on the same
    records one at a time. The MobileNet smoke config has window, closeness, edge mask and refine."""
    from mtl_ssl_amd import eval as ev, inference, input_reader, model_builder
    pictures = _pictures(SHAPES, 4)
    recs = _records(pictures)
    rec = str(tmp_path / "eval.record")
    input_reader.write_tfrecord(rec, recs)
    run = tmp_path / "run"
    run.mkdir()
    _state(config_name, str(run / "model.ckpt.npz"))
    for ema in (False, True):
        cfgp = _pipeline(tmp_path, config_name, ema, rec, len(recs))
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
        out = ev.main(["--checkpoint_dir=" + str(run), "--pipeline_config_path=" + cfgp])
        monkeypatch.setattr(model_builder, "build", real_build)
        assert out["num_images"] == len(recs) == len(captured)
        want = [inference.split_outputs(inference.output_tensors(d))[0] for d in captured]
        assert all(w["num_detections"] > 0 for w in want)
        det = inference.Detector(cfgp, str(run / "model.ckpt"), input_type="tf_example")
        assert det.moving_averages_applied == (len(model_builder.variable_specs(det.config.model)) if ema else 0)
        got = [det.detect_examples([r])[0] for r in recs]
        _assert_same(got, want, (config_name, ema))
        _untouched(det)
        del det
        torch.cuda.empty_cache()


def test_export_then_from_export_equals_the_source_checkpoint(tmp_path):
    from mtl_ssl_amd import inference
    name = "smoke_mobilenet_v1_mtl.config"
    src = _state(name, str(tmp_path / "model.ckpt.npz"))
    pictures = _pictures(SHAPES[:3], 6)
    results = {}
    for ema in (False, True):
        cfgp = _pipeline(tmp_path, name, ema)
        out = str(tmp_path / ("export_ema" if ema else "export"))
        r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.export_inference_graph",
                            "--pipeline_config_path=" + cfgp, "--trained_checkpoint_prefix=" + src[:-len(".npz")],
                            "--output_directory=" + out], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        direct = inference.Detector(cfgp, src)
        exported = inference.Detector.from_export(out)
        assert exported.input_type == "image_tensor" and exported.moving_averages_applied == 0
        a, b = direct(pictures), exported(pictures)
        _assert_same(a, b, ema)
        results[ema] = a
        del direct, exported
    # the shadows are other weights: the two exports do differ
    assert any(not np.array_equal(x["detection_scores"], y["detection_scores"]) for x, y in zip(results[0], results[1]))


def test_the_three_input_types_give_the_same_detections(tmp_path):
    from mtl_ssl_amd import inference
    name = "smoke_mobilenet_v1_mtl.config"
    src = _state(name, str(tmp_path / "model.ckpt.npz"))
    det = inference.Detector(_pipeline(tmp_path, name, False), src)
    pictures = _pictures(SHAPES, 8)
    encoded = [_png(p) for p in pictures]
    recs = _records(pictures)
    want = det.detect_images(pictures)
    _assert_same(det.detect_encoded(encoded), want, "encoded")
    _assert_same(det.detect_examples(recs), want, "tf_example")
    for kind, inputs in (("image_tensor", pictures), ("encoded_image_string_tensor", encoded), ("tf_example", recs)):
        det.input_type = kind
        _assert_same(det(inputs), want, kind)
    assert all(r["detection_boxes"].shape == (300, 4) for r in want)
    _untouched(det)


def test_mixed_sizes_match_one_at_a_time_calls(tmp_path):
    """Grouped by resized shape (here 4 images at 160x224 and one at 224x160) against B=1 calls: same counts and
    classes, scores and boxes within 1e-5 relative. The largest difference is printed."""
    from mtl_ssl_amd import inference
    name = "smoke_mobilenet_v1_mtl.config"
    src = _state(name, str(tmp_path / "model.ckpt.npz"))
    det = inference.Detector(_pipeline(tmp_path, name, False), src)
    sizes = [(160, 224), (224, 160), (150, 210), (160, 224), (120, 168)]
    assert sorted({det.resized_shape(h, w) for h, w in sizes}) == [(160, 224), (224, 160)]
    pictures = _pictures(sizes, 10)
    together = det.detect_images(pictures)
    single = [det.detect_images([p])[0] for p in pictures]
    worst = {"detection_scores": 0.0, "detection_boxes": 0.0}
    for i, (a, b) in enumerate(zip(together, single)):
        assert a["num_detections"] == b["num_detections"] > 0, i
        assert np.array_equal(a["detection_classes"], b["detection_classes"]), i
        for k in worst:
            scale = max(float(np.abs(b[k]).max()), 1e-30)
            d = float(np.abs(a[k] - b[k]).max()) / scale
            worst[k] = max(worst[k], d)
            assert d <= 1e-5, (i, k, d)
    print("mixed sizes vs one at a time: max relative difference scores %.3g boxes %.3g"
          % (worst["detection_scores"], worst["detection_boxes"]))
    # the batched form of one [B,H,W,3] array: the exporter's [B, ...] tensors
    same = np.stack([pictures[0], pictures[3]])
    batched = det.detect_images(same, batched=True)
    assert batched["detection_boxes"].shape == (2, 300, 4) and batched["num_detections"].shape == (2,)
    per = det.detect_images(same)
    _assert_same(inference.split_outputs(batched), per, "batched")
    _untouched(det)
