"""The VGG-16 family through the launchers, the way a user runs them: plain detection records -> `python -m
mtl_ssl_amd.train` (auxiliary labels generated on the device) -> `python -m mtl_ssl_amd.eval` -> export_inference_graph ->
Detector.from_export, whose detections equal eval's bit for bit at B = 1.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by module
name, and this runs with the end-to-end stage."""
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.vgg import vgg_ref

pytestmark = pytest.mark.gpu
ROOT = vgg_ref.ROOT
K, H, W = 5, 160, 224


def _records(n, rng):
    """Lossless (PNG) tf.Examples with two or three boxes of different classes each; every class occurs."""
    from PIL import Image
    from mtl_ssl_amd import input_reader as R
    recs = []
    for i in range(n):
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        base = np.stack([x / W * 255, y / H * 255, (x + y) / (H + W) * 255], -1)
        img = np.clip(base + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)
        G = 2 + i % 2
        cyx, hw = rng.uniform(0.3, 0.7, (G, 2)), rng.uniform(0.3, 0.5, (G, 2))
        b = np.concatenate([cyx - hw / 2, cyx + hw / 2], 1).clip(0, 1).astype(np.float32)
        cls = (i + np.arange(G)) % K
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        recs.append(R.serialize_example({
            "image/encoded": buf.getvalue(), "image/format": b"png", "image/filename": "im%d.png" % i,
            "image/source_id": str(i), "image/height": np.array([H]), "image/width": np.array([W]),
            "image/object/bbox/ymin": b[:, 0], "image/object/bbox/xmin": b[:, 1],
            "image/object/bbox/ymax": b[:, 2], "image/object/bbox/xmax": b[:, 3],
            "image/object/class/label": (cls + 1).astype(np.int64), "image/object/difficult": np.zeros(G, np.int64)}))
    return recs


def _run(args):
    r = subprocess.run([sys.executable, "-m"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (args[0], r.stderr[-3000:])
    return r


def test_train_eval_export_detect(tmp_path, monkeypatch):
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import eval as ev, inference, input_reader, model_builder
    recs = _records(6, np.random.RandomState(12))
    rec = str(tmp_path / "plain.record")
    input_reader.write_tfrecord(rec, recs)
    text = open(vgg_ref.SMOKE).read()
    text += 'train_input_reader { min_after_dequeue: 4 num_readers: 2 tf_record_input_reader { input_path: "%s" } }\n' % rec
    text += "eval_config { num_examples: %d }\n" % len(recs)
    text += 'eval_input_reader { shuffle: false tf_record_input_reader { input_path: "%s" } }\n' % rec
    cfgp = str(tmp_path / "pipeline.config")
    open(cfgp, "w").write(text)
    run = str(tmp_path / "run")
    r = _run(["mtl_ssl_amd.train", "--pipeline_config_path=" + cfgp, "--num_steps=3", "--train_dir=" + run,
              "--aux_labels=generate"])
    assert "auxiliary labels: generated on the device" in r.stdout and "global step 3" in r.stdout, r.stdout
    assert os.path.exists(os.path.join(run, "model.ckpt.npz"))
    r = _run(["mtl_ssl_amd.eval", "--checkpoint_dir=" + run, "--pipeline_config_path=" + cfgp,
              "--eval_dir=" + str(tmp_path / "eval")])
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and "mean_ap" in l]
    assert len(lines) == 1 and lines[0]["num_images"] == len(recs) and lines[0]["global_step"] == 3, r.stdout
    assert math.isfinite(lines[0]["mean_ap"]), lines[0]
    print("vgg_16 smoke: eval after 3 steps:", lines[0])
    out = str(tmp_path / "exported")
    _run(["mtl_ssl_amd.export_inference_graph", "--input_type=tf_example", "--pipeline_config_path=" + cfgp,
          "--trained_checkpoint_prefix=" + os.path.join(run, "model.ckpt"), "--output_directory=" + out])
    # eval's own loop (B = 1) in this process with its postprocess outputs captured: the Detector == eval claim
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
    res = ev.main(["--checkpoint_dir=" + run, "--pipeline_config_path=" + cfgp])
    monkeypatch.setattr(model_builder, "build", real_build)
    assert res["num_images"] == len(recs) == len(captured) and res["mean_ap"] == lines[0]["mean_ap"]
    want = inference.split_outputs(inference.output_tensors(captured[0]))[0]
    det = inference.Detector.from_export(out)
    assert det.input_type == "tf_example"
    got = det([recs[0]])[0]
    assert want["num_detections"] > 0 and sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype == np.float32 and np.array_equal(got[k], want[k]), k
    assert det.model.step == 0
