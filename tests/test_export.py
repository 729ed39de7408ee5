"""export_inference_graph and the host side of mtl_ssl_amd.inference, without a GPU: the reference's flags and errors,
the exported TF V2 bundle against the source state (plain and moving averages, strict about missing variables, from a
TF checkpoint too), the exporter's output contract, the decoder against input_reader's and the order of grouped
results."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "configs", "smoke_mobilenet_v1_mtl.config")


def _config(tmp_path, ema):
    text = open(CONFIG).read() + ("\neval_config { use_moving_averages: true }\n" if ema else "")
    p = str(tmp_path / ("pipeline_ema.config" if ema else "pipeline.config"))
    open(p, "w").write(text)
    return p


@pytest.fixture(scope="module")
def specs():
    from mtl_ssl_amd import config, model_builder
    cfg = config.parse_pipeline_config(open(CONFIG).read())
    return model_builder.variable_specs(cfg.model, is_training=False)


@pytest.fixture(scope="module")
def state(specs, tmp_path_factory):
    """A training state file as checkpoint.save writes it: variables, momentum slots, moving averages, step."""
    rng = np.random.RandomState(3)
    out = {}
    for s in specs:
        v = rng.standard_normal(s.shape).astype(np.float32)
        out[s.name] = v
        out[s.name + "/Momentum"] = v * 0.5
        out[s.name + "/ExponentialMovingAverage"] = v + 1.0
    out["global_step"] = np.asarray(17, np.int64)
    p = str(tmp_path_factory.mktemp("train") / "model.ckpt.npz")
    np.savez(p, **out)
    return p, out


def test_inference_variables_are_registered_on_the_host(specs):
    from mtl_ssl_amd import config, model_builder
    cfg = config.parse_pipeline_config(open(CONFIG).read())
    train = model_builder.variable_specs(cfg.model, is_training=True)
    assert [s.name for s in specs] == [s.name for s in train] and len(specs) == 169
    assert all(s.offset == -1 for s in specs)                                    # nothing was allocated
    assert specs[0].name.startswith("FirstStageFeatureExtractor/MobilenetV1/")


@pytest.mark.parametrize("missing", ["pipeline_config_path", "trained_checkpoint_prefix", "output_directory"])
def test_a_missing_flag_fails_with_the_reference_message(missing, tmp_path):
    from mtl_ssl_amd import export_inference_graph as X
    flags = {"pipeline_config_path": CONFIG, "trained_checkpoint_prefix": str(tmp_path / "model.ckpt"),
             "output_directory": str(tmp_path / "out")}
    del flags[missing]
    with pytest.raises(AssertionError, match="`%s` is missing" % missing):
        X.main(["--%s=%s" % kv for kv in flags.items()])
    assert not os.path.exists(tmp_path / "out")


def test_an_unknown_input_type_raises_the_reference_error(state, tmp_path):
    from mtl_ssl_amd import export_inference_graph as X
    with pytest.raises(ValueError, match=r"^Unknown input type: jpeg_files$"):
        X.main(["--input_type=jpeg_files", "--pipeline_config_path=" + CONFIG,
                "--trained_checkpoint_prefix=" + state[0], "--output_directory=" + str(tmp_path / "out")])
    assert not os.path.exists(tmp_path / "out")


def _read_bundle(out_dir):
    from mtl_ssl_amd import tf_checkpoint
    r = tf_checkpoint.open_tf_checkpoint(os.path.join(out_dir, "model.ckpt"), verify=True)
    return {k: r[k] for k in r.keys()}


@pytest.mark.parametrize("ema", [False, True])
def test_export_writes_the_inference_variables(ema, specs, state, tmp_path):
    """The CLI in a child process (no GPU needed): the bundle holds exactly the inference model's variables, their
    values (or their shadows), nothing of the optimizer; pipeline.config and export.json beside it."""
    path, src = state
    cfg = _config(tmp_path, ema)
    out = str(tmp_path / "exported" / "model")
    r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.export_inference_graph", "--input_type", "tf_example",
                        "--pipeline_config_path", cfg, "--trained_checkpoint_prefix", path[:-len(".npz")],
                        "--output_directory", out], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("saved_model/ are not written") == 1
    got = _read_bundle(out)
    assert sorted(got) == sorted(s.name for s in specs)
    for s in specs:
        want = src[s.name + "/ExponentialMovingAverage"] if ema else src[s.name]
        assert got[s.name].dtype == np.float32 and np.array_equal(got[s.name], want), s.name
    assert open(os.path.join(out, "pipeline.config")).read() == open(cfg).read()
    meta = json.load(open(os.path.join(out, "export.json")))
    assert meta == {"format_version": 1, "input_type": "tf_example", "trained_checkpoint_prefix": path[:-len(".npz")],
                    "use_moving_averages": ema, "moving_averages_applied": len(specs) if ema else 0,
                    "num_variables": len(specs)}
    assert sorted(os.listdir(out)) == ["export.json", "model.ckpt.data-00000-of-00001", "model.ckpt.index",
                                       "pipeline.config"]


def test_moving_averages_without_shadows_raise_the_eval_error(specs, state, tmp_path):
    from mtl_ssl_amd import checkpoint, export_inference_graph as X
    plain = {k: v for k, v in state[1].items() if not k.endswith("/ExponentialMovingAverage")}
    p = str(tmp_path / "model.ckpt.npz")
    np.savez(p, **plain)
    with pytest.raises(ValueError) as e:
        X.export_inference_graph("image_tensor", _config(tmp_path, True), p, str(tmp_path / "out"))
    assert str(e.value) == checkpoint.NO_MOVING_AVERAGES % p
    assert not os.path.exists(tmp_path / "out")
    # without use_moving_averages the same state exports
    assert X.export_inference_graph("image_tensor", _config(tmp_path, False), p, str(tmp_path / "out"))[
        "num_variables"] == len(specs)


def test_a_missing_variable_fails_and_is_named(specs, state, tmp_path):
    from mtl_ssl_amd import export_inference_graph as X
    gone = specs[len(specs) // 2].name
    p = str(tmp_path / "model.ckpt.npz")
    np.savez(p, **{k: v for k, v in state[1].items() if k != gone})
    with pytest.raises(KeyError, match=gone):
        X.export_inference_graph("image_tensor", _config(tmp_path, False), p, str(tmp_path / "out"))
    bad = dict(state[1])
    bad[gone] = np.zeros((3,), np.float32)
    np.savez(p, **bad)
    with pytest.raises(ValueError, match=gone):
        X.export_inference_graph("image_tensor", _config(tmp_path, False), p, str(tmp_path / "out"))
    assert not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("ema", [False, True])
def test_a_tensorflow_v2_prefix_exports_the_same_bundle(ema, specs, state, tmp_path):
    from mtl_ssl_amd import export_inference_graph as X, tf_checkpoint
    path, src = state
    tf_prefix = str(tmp_path / "tf" / "model.ckpt-17")
    os.makedirs(os.path.dirname(tf_prefix))
    tf_checkpoint.write_bundle(tf_prefix, src)
    cfg = _config(tmp_path, ema)
    X.export_inference_graph("image_tensor", cfg, tf_prefix, str(tmp_path / "from_tf"))
    X.export_inference_graph("image_tensor", cfg, path, str(tmp_path / "from_npz"))
    a, b = _read_bundle(str(tmp_path / "from_tf")), _read_bundle(str(tmp_path / "from_npz"))
    assert sorted(a) == sorted(b) == sorted(s.name for s in specs)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for name in ("model.ckpt.index", "model.ckpt.data-00000-of-00001"):
        assert open(tmp_path / "from_tf" / name, "rb").read() == open(tmp_path / "from_npz" / name, "rb").read()


def test_output_contract_adds_the_label_offset_and_floats_the_counts():
    from mtl_ssl_amd import inference
    post = {"detection_boxes": np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4) / 24,
            "detection_scores": np.asarray([[0.9, 0.5, 0.0], [0.7, 0.0, 0.0]], np.float32),
            "detection_classes": np.asarray([[0, 4, 0], [2, 0, 0]], np.float32),
            "num_detections": np.asarray([2, 1], np.int32)}
    out = inference.output_tensors(post)
    assert {k: v.dtype for k, v in out.items()} == {k: np.dtype(np.float32) for k in inference.OUTPUT_KEYS}
    assert np.array_equal(out["detection_classes"], [[1, 5, 1], [3, 1, 1]])
    assert np.array_equal(out["num_detections"], [2.0, 1.0])
    assert np.array_equal(out["detection_boxes"], post["detection_boxes"])
    per = inference.split_outputs(out)
    assert len(per) == 2 and per[1]["num_detections"] == np.float32(1) and isinstance(per[1]["num_detections"],
                                                                                       np.float32)
    assert per[0]["detection_boxes"].shape == (3, 4) and np.array_equal(per[1]["detection_classes"], [3, 1, 1])
    back = inference.stack_outputs(per)
    assert all(np.array_equal(back[k], out[k]) and back[k].dtype == np.float32 for k in out)
    with pytest.raises(ValueError, match="detection_classes"):
        inference.output_tensors({k: v for k, v in post.items() if k != "detection_classes"})


def _encode(arr, fmt, mode=None):
    from PIL import Image
    buf = io.BytesIO()
    im = Image.fromarray(arr, mode) if mode else Image.fromarray(arr)
    im.save(buf, format=fmt, **({"quality": 90} if fmt == "JPEG" else {}))
    return buf.getvalue()


def test_decoder_gives_the_input_readers_pixels():
    from mtl_ssl_amd import inference, input_reader
    rng = np.random.RandomState(1)
    cases = {"jpeg": _encode(rng.randint(0, 256, (37, 53, 3)).astype(np.uint8), "JPEG"),
             "png": _encode(rng.randint(0, 256, (21, 17, 3)).astype(np.uint8), "PNG"),
             "gray_png": _encode(rng.randint(0, 256, (19, 23)).astype(np.uint8), "PNG"),
             "gray_jpeg": _encode(rng.randint(0, 256, (16, 24)).astype(np.uint8), "JPEG"),
             "rgba_png": _encode(rng.randint(0, 256, (13, 29, 4)).astype(np.uint8), "PNG")}
    for name, enc in cases.items():
        ex = input_reader.serialize_example({"image/encoded": enc, "image/format": b"x"})
        want = input_reader.decode_example_uint8(ex, 3)["image"]
        for got in (inference.decode_image(enc), inference.image_from_example(ex)):
            assert got.dtype == np.uint8 and got.shape == want.shape and want.shape[2] == 3, name
            assert np.array_equal(got, want), name
    gray = np.asarray(inference.decode_image(cases["gray_png"]))
    assert np.array_equal(gray[..., 0], gray[..., 2])
    rgba = rng.randint(0, 256, (5, 6, 4)).astype(np.uint8)
    assert np.array_equal(inference.decode_image(_encode(rgba, "PNG")), rgba[..., :3])   # alpha dropped
    with pytest.raises(ValueError, match="BMP"):
        inference.decode_image(_encode(rgba[..., :3].copy(), "BMP"))
    with pytest.raises(ValueError, match="JPEG or PNG"):
        inference.decode_image(b"not an image")
    with pytest.raises(ValueError, match="image/encoded"):
        inference.image_from_example(input_reader.serialize_example({"image/format": b"jpeg"}))


def test_grouped_results_come_back_in_input_order():
    from mtl_ssl_amd import inference
    keys = [(600, 800), (800, 600), (600, 800), (512, 512), (800, 600), (600, 800)]
    calls = []

    def run_group(idx, key):
        calls.append((key, list(idx)))
        return [("r", i, key) for i in idx]
    out = inference.run_grouped(keys, run_group)
    assert out == [("r", i, k) for i, k in enumerate(keys)]
    assert calls == [((600, 800), [0, 2, 5]), ((800, 600), [1, 4]), ((512, 512), [3])]
    with pytest.raises(RuntimeError):
        inference.run_grouped(keys, lambda idx, key: [0])
    assert inference.run_grouped([], run_group) == []


def test_detector_refuses_an_unknown_input_type():
    from mtl_ssl_amd import inference
    with pytest.raises(ValueError, match="^Unknown input type: bytes$"):
        inference.Detector(CONFIG, "unused", input_type="bytes")
