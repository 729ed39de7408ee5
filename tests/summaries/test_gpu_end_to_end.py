"""The summaries end to end on the GPU: trainer.train leaves the run bit-identical with summaries on or off and an event
file whose histograms are those of the saved weights; python -m mtl_ssl_amd.eval --eval_dir writes the scalars of its
metrics file and an image per visualisation.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage."""
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _train(tmp_path, name, secs, capsys):
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "smoke_mobilenet_v1_mtl.config")).read())
    batch = synthetic.make_batch(2, 160, 224, 5, seed=3, device="cuda", max_gt=4, num_windows=6)
    d = str(tmp_path / name)
    tr, log = trainer.train(lambda: batch, lambda: model_builder.build(cfg.model, True, "cuda", seed=1), cfg.train_config,
                            train_dir=d, num_steps=3, model_config=cfg.model, log_every=1, save_summaries_secs=secs)
    return d, tr, log, capsys.readouterr().out


def test_training_is_bit_identical_with_summaries_and_the_histograms_are_the_saved_weights(tmp_path, capsys):
    from mtl_ssl_amd import summaries
    d_on, tr, log_on, out_on = _train(tmp_path, "on", 1e-9, capsys)            # a summary at every (log) step
    d_off, _, log_off, out_off = _train(tmp_path, "off", 0, capsys)
    strip = lambda s: re.sub(r"\(\d+\.\d+ sec/step\)", "", s)
    assert strip(out_on) == strip(out_off) and out_on.count("global step") == 3
    assert [e["loss"] for e in log_on] == [e["loss"] for e in log_off]
    assert open(os.path.join(d_on, "model.ckpt.npz"), "rb").read() == open(os.path.join(d_off, "model.ckpt.npz"), "rb").read()
    assert summaries.event_files(d_off) == []
    (path,) = summaries.event_files(d_on)
    ev = summaries.read_events(path)
    assert ev[0]["file_version"] == "brain.Event:2" and {e["step"] for e in ev[1:]} == {1, 2, 3}
    last = [v for e in ev if e["step"] == 3 for v in e["values"]]
    scalars = {v["tag"]: v["simple_value"] for v in last if "simple_value" in v}
    histos = {v["tag"]: v["histo"] for v in last if "histo" in v}
    loss_tags = sorted(t for t in scalars if t.startswith("Loss/"))
    assert len(loss_tags) >= 4 and {"TotalLoss", "Learning_Rate", "global_step/sec"} <= set(scalars)
    total = sum(scalars[t] for t in loss_tags)
    assert np.float32(total) == pytest.approx(log_on[-1]["loss"], rel=1e-5) and scalars["TotalLoss"] >= total * (1 - 1e-6)
    state = np.load(os.path.join(d_on, "model.ckpt.npz"))
    assert sorted(histos) == sorted(s.name for s in tr.ps.specs)
    for s in tr.ps.specs:
        m, c = summaries.histogram_numpy(state[s.name])
        bl, bc = summaries.encode_histogram(c)
        h = histos[s.name]
        assert h["bucket_limit"] == bl and h["bucket"] == bc, s.name
        assert (h["min"], h["max"], h["num"]) == (m[0], m[1], m[2]), s.name
        # two double sums of the same non-negative terms in different orders: each within n * 2^-53 of the exact one
        assert abs(h["sum_squares"] - m[4]) <= 2 * s.size * 2.0 ** -53 * m[4], s.name


def test_eval_writes_the_scalars_of_its_metrics_file_and_the_drawn_images(tmp_path):
    from mtl_ssl_amd import summaries
    from tests.eval_workflow.test_gpu_end_to_end import FRCNN, H, W, _config, _eval_main, _run_dir, _write_records
    rec = str(tmp_path / "voc.record")
    _write_records(rec, [2, 1], 31)
    run = _run_dir(tmp_path, FRCNN)
    vis, eval_dir = str(tmp_path / "vis"), str(tmp_path / "eval")
    opts = 'calc_loss: true num_visualizations: 1 visualization_export_dir: "%s"' % vis
    out = _eval_main(run, _config(tmp_path, FRCNN, rec, opts), "--eval_dir=" + eval_dir)
    metrics = json.load(open(os.path.join(eval_dir, "metrics-3.json")))
    (path,) = summaries.event_files(eval_dir)
    ev = summaries.read_events(path)
    assert ev[0]["file_version"] == "brain.Event:2" and {e["step"] for e in ev[1:]} == {3}
    values = [v for e in ev[1:] for v in e["values"]]
    scalars = [(v["tag"], v["simple_value"]) for v in values if "simple_value" in v]
    want = sorted(k for k, v in metrics.items() if isinstance(v, (int, float)) and not isinstance(v, bool))
    assert [t for t, _ in scalars] == want                       # exactly the scalar keys, sorted
    assert any(t.startswith("Loss/") for t in want) and any(t.startswith("mtl/") for t in want) and "mean_ap" in want
    for tag, got in scalars:
        w = np.float32(metrics[tag])
        assert (np.isnan(w) and np.isnan(got)) or np.float32(got) == w, (tag, got, metrics[tag])
    images = [v for v in values if "image" in v]
    assert [v["tag"] for v in images] == ["2008_000000.png/image"]
    png = open(os.path.join(vis, "export-2008_000000.png.png"), "rb").read()
    assert images[0]["image"] == {"height": H, "width": W, "colorspace": 3, "encoded_image_string": png}
    assert len(values) == len(scalars) + 1 and out["global_step"] == 3
