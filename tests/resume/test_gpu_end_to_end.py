"""Stopping and resuming on the GPU: a run cut in two must end in the bits of the run that was never cut. First the
trainer's own state (weights, optimizer slots, moving averages, step: whatever a step reads must be in the state file
or be recomputed by prepare() exactly), on a fixed ring of synthetic batches so that no input stream is involved; then
record-fed runs through the launcher, where the input stream's state travels in the same file; then the device
preparer alone. Every comparison is equality.

The module shares its name with tests/test_gpu_end_to_end.py on purpose: tests/conftest.py orders the GPU suite by
module name, and these run with the end-to-end stage."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.aux_labels.test_gpu_end_to_end import _write_plain_records
from tests.test_input_pipeline import K as PIPE_K
from tests.test_input_pipeline import SHAPES as PIPE_SHAPES
from tests.test_input_pipeline import _example
from tests.test_input_state import LOOPED, PHOTOMETRIC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, W, K = 64, 96, 5
ADAM = "adam_optimizer { learning_rate { constant_learning_rate { learning_rate: 0.0001 } } }"


def _config_text(name):
    text = open(os.path.join(ROOT, "configs", name)).read()
    small = "min_dimension: %d max_dimension: %d" % (H, W)
    assert "min_dimension: 160 max_dimension: 224" in text
    return text.replace("min_dimension: 160 max_dimension: 224", small)


def _frcnn_momentum_ema_dropout():
    text = _config_text("smoke_resnet50_mtl.config")
    assert "use_moving_average: false" in text and "refine_num_fc_layers: 0" in text
    text = text.replace("use_moving_average: false", "use_moving_average: true moving_average_decay: 0.9")
    return text.replace("refine_num_fc_layers: 0", "refine_num_fc_layers: 2  refine_dropout_rate: 0.7"), "record"


def _rfcn_adam():
    text = _config_text("smoke_rfcn_resnet50_mtl.config")
    text, n = re.subn(r"optimizer \{.*use_moving_average: false \}", "optimizer { %s use_moving_average: false }" % ADAM,
                      text, flags=re.S)
    assert n == 1
    return text, "record"


def _mobilenet_generated_labels():
    return _config_text("smoke_mobilenet_v1_mtl.config"), "generate"


@pytest.mark.parametrize("case", [_frcnn_momentum_ema_dropout, _rfcn_adam, _mobilenet_generated_labels],
                         ids=["frcnn_momentum_ema_dropout", "rfcn_adam", "mobilenet_generated_labels"])
def test_trainer_state_round_trip_is_exact(case, tmp_path):
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import checkpoint, config, model_builder, synthetic, trainer
    text, aux = case()
    cfg = config.parse_pipeline_config(text)
    ring = [synthetic.make_batch(2, H, W, K, seed=20 + i, device="cuda", max_gt=4, num_windows=6) for i in range(4)]

    def fresh():
        model = model_builder.build(cfg.model, True, "cuda", seed=1)
        return model, trainer.Trainer(model, cfg.train_config, 1, aux_labels=aux, aux_num_windows=6)

    def steps(tr, batches):
        out = []
        for b in batches:
            losses = tr.step(b)
            torch.cuda.synchronize()
            out.append({k: float(v.item()) for k, v in losses.items()})
        return out

    model, tr = fresh()
    whole = steps(tr, ring)
    checkpoint.save(str(tmp_path / "a.npz"), model.ps, tr.global_step, tr)
    model, tr = fresh()
    halves = steps(tr, ring[:2])
    checkpoint.save(str(tmp_path / "mid.npz"), model.ps, tr.global_step, tr)
    del model, tr
    model, tr = fresh()
    tr.global_step = checkpoint.load(str(tmp_path / "mid.npz"), model.ps, tr)
    model.prepare()
    assert tr.global_step == 2
    halves += steps(tr, ring[2:])
    checkpoint.save(str(tmp_path / "b.npz"), model.ps, tr.global_step, tr)
    assert all(np.isfinite(v) for s in whole for v in s.values())
    assert halves == whole
    a, b = np.load(str(tmp_path / "a.npz")), np.load(str(tmp_path / "b.npz"))
    assert sorted(a.files) == sorted(b.files) and int(b["global_step"]) == 4
    differing = [k for k in a.files if not np.array_equal(a[k], b[k])]
    assert not differing, differing[:10]
    mid = np.load(str(tmp_path / "mid.npz"))
    assert any(not np.array_equal(a[k], mid[k]) for k in a.files if k.endswith("/weights"))     # the last two steps moved them


# ------------------------------------------------------------------------------------------ record-fed runs, launcher
RECORD_SHAPES = [(64, 96), (96, 64), (64, 64), (64, 96), (96, 64), (64, 64), (48, 72), (64, 96), (96, 64), (64, 64),
                 (72, 48), (48, 72)]
LOSS_LINE = re.compile(r"global step (\d+): loss = (\S+)")


def _launch(train_dir, cfgp, num_steps, *more):
    r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.train", "--train_dir=" + train_dir,
                        "--pipeline_config_path=" + cfgp, "--num_steps=%d" % num_steps, "--aux_labels=generate",
                        "--log_every=1", "--save_summaries_secs=0"] + list(more),
                       env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """A: six steps in one go. B: three steps, then three more. C: B's first half, continued with --input_state=restart.
    D: B's first half, one more step from the host generator. -> {name: (train_dir, stdout of its last launch)}"""
    import __graft_entry__ as g
    g.build()
    d = tmp_path_factory.mktemp("resume")
    rec = str(d / "train.record")
    _write_plain_records(rec, RECORD_SHAPES, K, np.random.RandomState(6))
    text = _config_text("smoke_mobilenet_v1_mtl.config")
    flip = "data_augmentation_options { random_horizontal_flip { } }"
    assert flip in text and "batch_size: 2" in text
    text = text.replace(flip, flip + """
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 255 target_minval: 0 target_maxval: 1 } }
  data_augmentation_options { random_adjust_brightness { max_delta: 0.3 } }
  data_augmentation_options { normalize_image { original_minval: 0 original_maxval: 1 target_minval: 0 target_maxval: 255 } }""")
    text += '\ntrain_input_reader { shuffle: true min_after_dequeue: 3 tf_record_input_reader { input_path: "%s" } }\n' % rec
    cfgp = str(d / "pipeline.config")
    open(cfgp, "w").write(text)
    from mtl_ssl_amd import config
    from mtl_ssl_amd.frcnn import FasterRCNNMetaArch as M
    rz = config.parse_pipeline_config(text).model.faster_rcnn.image_resizer
    assert {M.resized_shape(h, w, rz) for h, w in RECORD_SHAPES} == {(H, W), (W, H), (H, H)}      # three buckets
    dirs = {n: str(d / n) for n in "ABCD"}
    out = {"A": _launch(dirs["A"], cfgp, 6)}
    _launch(dirs["B"], cfgp, 3)
    shutil.copytree(dirs["B"], dirs["C"])
    shutil.copytree(dirs["B"], dirs["D"])
    out["B"] = _launch(dirs["B"], cfgp, 6)
    out["C"] = _launch(dirs["C"], cfgp, 6, "--input_state=restart")
    out["D"] = _launch(dirs["D"], cfgp, 4, "--input_pipeline=host")
    return {n: (dirs[n], out[n]) for n in "ABCD"}


def _state(train_dir):
    return np.load(os.path.join(train_dir, "model.ckpt.npz"), allow_pickle=False)


def _losses(stdout):
    return {int(m.group(1)): m.group(0) for m in LOSS_LINE.finditer(stdout)}


def test_record_fed_run_resumes_exactly(runs):
    """The loss lines are compared up to the loss: a line ends in the wall-clock seconds of its step."""
    a, b = _state(runs["A"][0]), _state(runs["B"][0])
    assert sorted(a.files) == sorted(b.files) and "input_state/rank0" in a.files and int(a["input_state/world"]) == 1
    differing = [k for k in a.files if not np.array_equal(a[k], b[k])]
    assert not differing, differing[:10]
    la, lb = _losses(runs["A"][1]), _losses(runs["B"][1])
    assert sorted(lb) == [4, 5, 6] and sorted(la) == [1, 2, 3, 4, 5, 6]
    assert [lb[s] for s in (4, 5, 6)] == [la[s] for s in (4, 5, 6)]
    st = json.loads(a["input_state/rank0"].tobytes().decode("utf-8"))
    assert st["batches"] == 6 and len(st["shuffle"]) == 3 and len(st["definition"]["options"]) == 4
    assert "restarts at its first record" not in runs["B"][1]


def test_input_state_restart_flag(runs):
    a, c = _state(runs["A"][0]), _state(runs["C"][0])
    assert int(c["global_step"]) == 6 and sorted(a.files) == sorted(c.files)
    assert any(not np.array_equal(a[k], c[k]) for k in a.files if k.endswith("/weights"))
    assert "input stream of rank 0 restarts at its first record: --input_state=restart" in runs["C"][1]
    st = json.loads(c["input_state/rank0"].tobytes().decode("utf-8"))
    assert st["batches"] == 3                                        # the restarted stream has handed out three batches


def test_host_generator_warns_that_it_restarts(runs):
    d, stdout = runs["D"]
    assert "--input_pipeline=host cannot continue its input stream" in stdout and "global step 4" in stdout
    # its file still says where the restarted stream stands (a pipeline follows the generator): one batch from the start
    st = _state(d)
    assert int(st["global_step"]) == 4 and json.loads(st["input_state/rank0"].tobytes().decode("utf-8"))["batches"] == 1


# ------------------------------------------------------------------------------------------------- device preparer
def test_device_preparer_resumes_exactly(tmp_path):
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import input_pipeline as IP
    from mtl_ssl_amd import input_reader as R
    rng = np.random.RandomState(3)
    rec = str(tmp_path / "part.record")
    R.write_tfrecord(rec, [_example(rng, i, h, w) for i, (h, w) in enumerate(PIPE_SHAPES)])
    kw = dict(LOOPED, augmentation_options=PHOTOMETRIC, device="cuda", num_workers=2, prefetch=2)
    with IP.InputPipeline([rec], PIPE_K, rng=np.random.RandomState(7), **kw) as pipe:
        head = [next(pipe) for _ in range(3)]
        st = json.loads(json.dumps(pipe.state()))
        want = [next(pipe) for _ in range(4)]
    with IP.InputPipeline([rec], PIPE_K, state=st, **kw) as pipe:
        got = [next(pipe) for _ in range(4)]
    assert sum(len(b["items"]) for b in st["buckets"]) >= 1 and head[0]["images"].is_cuda
    for g_, w_ in zip(got, want):
        assert g_["images"].is_cuda and torch.equal(g_["images"], w_["images"])
        assert list(g_) == list(w_)
        for k in w_:
            if k != "images":
                assert len(g_[k]) == len(w_[k]) and all(
                    (a == b) if isinstance(b, str) else np.array_equal(a, b) for a, b in zip(g_[k], w_[k])), k
