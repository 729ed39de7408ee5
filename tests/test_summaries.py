"""Host side of the training / evaluation summaries (mtl_ssl_amd/summaries.py): TensorFlow's default histogram buckets,
the float64 restatement of Histogram::Add that the device kernel is tested against, the run-collapsing proto encoding,
the event-file writer and reader, and trainer.train's plumbing on a store that lives on the CPU."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38, np.float32(1e-12)], np.float32)


def test_default_bucket_limits():
    from mtl_ssl_amd import summaries
    lim = summaries.default_bucket_limits()
    assert lim.dtype == np.float64 and lim.shape == (1551,)
    assert (np.diff(lim) > 0).all()
    assert lim[775] == 0.0 and lim[776] == 1e-12 and lim[-1] == sys.float_info.max and lim[0] == -sys.float_info.max


def test_numpy_restatement_and_encoder_on_a_known_answer():
    from mtl_ssl_amd import summaries
    lim = summaries.default_bucket_limits()
    moments, counts = summaries.histogram_numpy(SPECIAL)
    assert counts.dtype == np.uint32 and counts.shape == (1551,)
    want = np.zeros(1551, np.uint32)
    want[776] = 4            # 0.0, -0.0, the smallest denormal and float32(1e-12) < 1e-12: first limit above is 1e-12
    want[775] = 1            # -1e-45: the first limit strictly greater is 0.0
    # -3e38 lies below every limit but -DBL_MAX: the first bucket a value can fall into is index 1 (index 0 ends at
    # -DBL_MAX, and no double is smaller than that, so upper_bound never returns it)
    want[1] = 1
    want[1550] = 1           # 3e38: only DBL_MAX, the last limit, is greater
    np.testing.assert_array_equal(counts, want)
    assert lim[0] == -sys.float_info.max and -1e20 < lim[1] < -9e19 and lim[1550] == sys.float_info.max
    x = SPECIAL.astype(np.float64)
    assert moments[0] == x.min() and moments[1] == x.max() and moments[2] == 7 and moments[5] == 0
    assert moments[3] == math.fsum(x) and moments[4] == pytest.approx(math.fsum(x * x), rel=1e-15)
    # EncodeToProto(preserve_zero_buckets=false)
    bl, bc = summaries.encode_histogram(counts, lim)
    assert len(bl) == len(bc) and sum(bc) == moments[2]
    assert bl[-1] == lim[-1]
    for a, b in zip(bc[:-1], bc[1:]):
        assert not (a == 0 and b == 0), "two zero-count entries in a row: a run was not collapsed"
    for limit, count in zip(bl, bc):
        i = int(np.flatnonzero(lim == limit)[0])
        assert counts[i] == count
        if count == 0:             # a collapsed run carries its LAST limit: the next bucket is occupied or the table ends
            assert i == len(lim) - 1 or counts[i + 1] > 0
    assert [c for c in bc if c] == [1, 1, 4, 1]
    # non-finite values are counted apart and leave everything else alone
    m2, c2 = summaries.histogram_numpy(np.concatenate([SPECIAL, np.float32([np.nan, np.inf, -np.inf])]))
    np.testing.assert_array_equal(c2, counts)
    assert m2[5] == 3 and (m2[:5] == moments[:5]).all()
    m0, c0 = summaries.histogram_numpy(np.zeros(0, np.float32))
    assert m0[0] == sys.float_info.max and m0[1] == -sys.float_info.max and m0[2] == 0 and not c0.any()


def _write_all_kinds(logdir):
    from mtl_ssl_amd import summaries
    lim = summaries.default_bucket_limits()
    values = (np.random.RandomState(0).standard_normal(1000) * 0.09).astype(np.float32)
    moments, counts = summaries.histogram_numpy(values)
    png = b"\x89PNG\r\n\x1a\n" + bytes(range(256))
    with summaries.SummaryWriter(logdir) as w:
        w.add_scalar("Loss/a", 0.1, 7)
        w.add_histogram("var/weights", moments, counts, lim, 7)
        w.add_text("ModelConfig", "model&nbsp;{<br>}", 0)
        w.add_image("im0/image", png, 12, 34, 7)
        w.flush()
        path = w.path
    return path, moments, counts, png


def test_writer_and_reader_round_trip(tmp_path):
    import re
    import socket
    from mtl_ssl_amd import summaries
    path, moments, counts, png = _write_all_kinds(str(tmp_path))
    assert re.fullmatch(r"events\.out\.tfevents\.\d{10}\." + re.escape(socket.gethostname()), os.path.basename(path))
    assert summaries.event_files(str(tmp_path)) == [path]
    ev = summaries.read_events(path)
    assert len(ev) == 5
    assert ev[0]["file_version"] == "brain.Event:2" and ev[0]["wall_time"] > 1e9 and not ev[0]["values"]
    (s,), (h,), (t,), (i,) = (e["values"] for e in ev[1:])
    assert [e["step"] for e in ev[1:]] == [7, 7, 0, 7]
    assert s == {"tag": "Loss/a", "simple_value": float(np.float32(0.1))}
    assert h["tag"] == "var/weights"
    bl, bc = summaries.encode_histogram(counts)
    assert h["histo"]["bucket_limit"] == bl and h["histo"]["bucket"] == bc
    for k, name in enumerate(("min", "max", "num", "sum", "sum_squares")):
        assert h["histo"][name] == moments[k]
    assert t["tag"] == "ModelConfig" and t["plugin_name"] == "text"
    assert t["tensor"] == {"dtype": 7, "string_val": [b"model&nbsp;{<br>}"]}
    assert i == {"tag": "im0/image", "image": {"height": 12, "width": 34, "colorspace": 3, "encoded_image_string": png}}
    # one flipped byte anywhere — length, either CRC or payload — is caught
    data = open(path, "rb").read()
    first = 8 + 4 + len(summaries.read_records(path)[0]) + 4
    for pos in (0, 9, 14, first + 3, first + 20, len(data) - 2):
        bad = bytearray(data)
        bad[pos] ^= 0x10
        p = str(tmp_path / "bad")
        open(p, "wb").write(bytes(bad))
        with pytest.raises(IOError):
            summaries.read_events(p)
    with pytest.raises(FloatingPointError, match="Nan in summary histogram for: v/bad"):
        m = moments.copy()
        m[5] = 1
        with summaries.SummaryWriter(str(tmp_path / "nan")) as w:
            w.add_histogram("v/bad", m, counts, summaries.default_bucket_limits(), 0)


def test_a_record_decodes_with_protobufs_own_wire_decoder(tmp_path):
    """A second opinion on the encoding: google.protobuf's descriptor-free primitives walk the histogram event."""
    decoder = pytest.importorskip("google.protobuf.internal.decoder", reason="google.protobuf is not installed")
    from mtl_ssl_amd import summaries
    import struct
    path, moments, counts, _ = _write_all_kinds(str(tmp_path))
    payload = summaries.read_records(path)[2]

    def walk(buf):
        """[(field number, wire type, value)] with protobuf's own varint decoder."""
        out, pos = [], 0
        while pos < len(buf):
            key, pos = decoder._DecodeVarint(buf, pos)
            fn, wt = key >> 3, key & 7
            if wt == 0:
                v, pos = decoder._DecodeVarint(buf, pos)
            elif wt == 1:
                v, pos = struct.unpack("<d", buf[pos:pos + 8])[0], pos + 8
            elif wt == 5:
                v, pos = struct.unpack("<f", buf[pos:pos + 4])[0], pos + 4
            else:
                assert wt == 2, wt
                n, pos = decoder._DecodeVarint(buf, pos)
                v, pos = buf[pos:pos + n], pos + n
                assert len(v) == n
            out.append((fn, wt, v))
        return out

    event = walk(payload)
    assert [(fn, wt) for fn, wt, _ in event] == [(1, 1), (2, 0), (5, 2)] and event[1][2] == 7
    (fn, wt, value), = walk(event[2][2])
    assert (fn, wt) == (1, 2)
    fields = walk(value)
    assert fields[0] == (1, 2, b"var/weights") and fields[1][:2] == (5, 2)
    histo = walk(fields[1][2])
    assert [fn for fn, _, _ in histo] == [1, 2, 3, 4, 5, 6, 7]
    assert [v for _, _, v in histo[:5]] == list(moments[:5])
    bl, bc = summaries.encode_histogram(counts)
    assert np.frombuffer(histo[5][2], "<f8").tolist() == bl and np.frombuffer(histo[6][2], "<f8").tolist() == bc


def _cpu_model(cfg):
    """The smoke MobileNet model with its store on the CPU: every variable registered and initialised, no device
    work (model_builder.build would go on to fold the BatchNorm scales on the GPU)."""
    from mtl_ssl_amd import model_builder
    model, ps = model_builder._construct(cfg.model, True, 2)
    ps.finalize("cpu", seed=2)
    return model


def _cpu_train(tmp_path, monkeypatch, name, secs, capsys):
    """trainer.train over a model whose store lives on the CPU; the step itself (device kernels) is replaced by a
    deterministic stand-in that moves the weights and returns loss scalars."""
    import torch
    from mtl_ssl_amd import config, model_builder, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "smoke_mobilenet_v1_mtl.config")).read())

    def step(self, batch):
        self.ps.weights.mul_(0.75)
        self.global_step += 1
        return {"first_stage_localization_loss": torch.tensor(0.5 / self.global_step),
                "second_stage_classification_loss": torch.tensor(0.125)}

    monkeypatch.setattr(trainer.Trainer, "step", step)
    monkeypatch.setattr(trainer.Trainer, "broadcast_weights", lambda self, root=0: None)
    d = str(tmp_path / name)
    tr, log = trainer.train(lambda: None, lambda: _cpu_model(cfg), cfg.train_config,
                            train_dir=d, num_steps=3, model_config=cfg.model, log_every=1, save_summaries_secs=secs,
                            total_configs=(cfg.model, cfg.train_config, cfg.get("train_input_reader")))
    return d, tr, capsys.readouterr().out


def test_train_writes_one_event_file_and_leaves_the_run_alone(tmp_path, monkeypatch, capsys):
    import re
    from mtl_ssl_amd import summaries
    d_on, tr, out_on = _cpu_train(tmp_path, monkeypatch, "on", 1e9, capsys)
    d_off, _, out_off = _cpu_train(tmp_path, monkeypatch, "off", 0, capsys)
    strip = lambda s: re.sub(r"\(\d+\.\d+ sec/step\)", "", s)
    assert strip(out_on) == strip(out_off) and "global step 3" in out_on
    assert open(os.path.join(d_on, "model.ckpt.npz"), "rb").read() == open(os.path.join(d_off, "model.ckpt.npz"), "rb").read()
    assert summaries.event_files(d_off) == []
    files = summaries.event_files(d_on)
    assert len(files) == 1
    ev = summaries.read_events(files[0])
    assert ev[0]["file_version"] == "brain.Event:2"
    values = [(e["step"], v) for e in ev[1:] for v in e["values"]]
    texts = {v["tag"]: v for _, v in values if "tensor" in v}
    assert sorted(texts) == ["EvalConfig", "EvalInputConfig", "ModelConfig", "TrainConfig", "TrainInputConfig"]
    assert b"faster_rcnn&nbsp;{<br>" in texts["ModelConfig"]["tensor"]["string_val"][0]
    assert texts["EvalConfig"]["tensor"]["string_val"] == [b""]
    # one summary: after the first completed step (the interval never elapses afterwards)
    scalars = {v["tag"]: (s, v["simple_value"]) for s, v in values if "simple_value" in v}
    assert {s for s, _ in scalars.values()} == {1}
    assert scalars["Loss/first_stage_localization_loss"][1] == 0.5
    assert scalars["Loss/second_stage_classification_loss"][1] == 0.125
    assert "Learning_Rate" in scalars and "TotalLoss" in scalars and "global_step/sec" in scalars
    ps = tr.ps
    histos = {v["tag"]: v["histo"] for _, v in values if "histo" in v}
    assert sorted(histos) == sorted(s.name for s in ps.specs) and len(histos) == len(ps.specs) > 10
    # the histograms are those of the weights after step 1: the saved ones (after step 3) scaled back, exactly
    # (0.75 is a power-of-two-friendly factor only for some values, so restate from the initial values instead)
    from mtl_ssl_amd import config, model_builder
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "smoke_mobilenet_v1_mtl.config")).read())
    ref = _cpu_model(cfg).ps
    ref.weights.mul_(0.75)
    reg = 0.0
    for s in ps.specs:
        m, c = summaries.histogram_numpy(ref.value(s.name).numpy())
        bl, bc = summaries.encode_histogram(c)
        h = histos[s.name]
        assert h["bucket_limit"] == bl and h["bucket"] == bc and h["num"] == s.size == m[2], s.name
        assert (h["min"], h["max"], h["sum"], h["sum_squares"]) == (m[0], m[1], m[3], m[4]), s.name
        reg += 0.5 * s.weight_decay * m[4] if s.trainable else 0.0
    assert reg > 0
    assert scalars["TotalLoss"][1] == pytest.approx(0.5 + 0.125 + reg, rel=1e-6)


def test_pipeline_config_accepts_the_summary_fields():
    from mtl_ssl_amd import config
    cfg = config.parse_pipeline_config("train_config { save_summaries_secs: 30 show_image_summary: true }")
    assert cfg.train_config.save_summaries_secs == 30 and cfg.train_config.show_image_summary is True
    cfg = config.parse_pipeline_config("train_config { batch_size: 2 }")
    assert cfg.train_config.save_summaries_secs == 120 and cfg.train_config.show_image_summary is False
