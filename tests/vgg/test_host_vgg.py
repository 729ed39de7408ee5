"""The VGG-16 extractor without a GPU: the variables the builder registers, the freeze_layer table and the refusals, the
classification-checkpoint round trip through the TF V2 container, export, and the test oracle's own geometry."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.vgg import vgg_ref

ROOT = vgg_ref.ROOT
SMOKE = vgg_ref.SMOKE
TRUNK = "FirstStageFeatureExtractor/vgg_16/"


def _cfg(fe_fields=None, text=None):
    from mtl_ssl_amd import config
    text = open(SMOKE).read() if text is None else text
    if fe_fields is not None:
        old = "feature_extractor { type: 'faster_rcnn_vgg_16' weight_decay: 0.0005 freeze_layer: 'conv1' }"
        assert old in text
        text = text.replace(old, "feature_extractor { type: 'faster_rcnn_vgg_16' %s }" % fe_fields)
    return config.parse_pipeline_config(text)


def test_builder_registers_the_26_trunk_variables_and_no_tower():
    """Fails before the extractor exists with "Unknown Faster R-CNN feature_extractor: faster_rcnn_vgg_16"."""
    from mtl_ssl_amd import model_builder
    specs = model_builder.variable_specs(_cfg().model, is_training=True)
    want = vgg_ref.trunk_names()
    assert len(want) == 26
    assert [(s.name, s.shape) for s in specs[:26]] == want                     # registration order, shapes
    assert not [s.name for s in specs[26:] if s.name.startswith(TRUNK)]
    for s in specs[:26]:
        assert s.weight_decay == (0.0005 if s.name.endswith("/weights") else 0.0), s.name
        assert s.init == (("variance_scaling", 1.0, "FAN_AVG", True) if s.name.endswith("/weights") else ("zeros",))
    names = [s.name for s in specs]
    for scope in ("SecondStageFeatureExtractor", "WindowBoxPredictor/vgg_16", "ClosenessBoxPredictor/vgg_16"):
        assert not [n for n in names if n.startswith(scope)], scope
    by = {s.name: s for s in specs}
    for scope in ("SecondStageBoxPredictor", "WindowBoxPredictor", "ClosenessBoxPredictor"):
        assert by[scope + "/FC_0_64/weights"].shape == (7 * 7 * 512, 64)
    assert by["SecondStageBoxPredictor/ClassPredictor/weights"].shape == (64, 6)
    # a config that does not set weight_decay gets the constructor's default
    d = model_builder.variable_specs(_cfg("freeze_layer: ''").model, True)
    assert d[0].weight_decay == 0.0005 and d[1].weight_decay == 0.0
    # the inference model holds the same variables
    assert [s.name for s in model_builder.variable_specs(_cfg().model, False)] == names


def test_both_shipped_vgg_configs_build():
    """configs/vgg16/ holds this family's two configurations (the eight directly under configs/ are the set that
    tests/test_host_logic.py pins): each parses and builds its whole variable set through the registry."""
    from mtl_ssl_amd import config, frcnn, model_builder, trainer
    cdir = os.path.join(ROOT, "configs", "vgg16")
    assert sorted(os.listdir(cdir)) == ["frcnn_vgg16_voc_mtl.config", "smoke_vgg16_mtl.config"]
    for f, n_vars, fc_in, fc_out, n_fc in (("frcnn_vgg16_voc_mtl.config", 56, 7 * 7 * 512, 4096, 2),
                                           ("smoke_vgg16_mtl.config", 50, 7 * 7 * 512, 64, 1)):
        cfg = config.parse_pipeline_config(open(os.path.join(cdir, f)).read())
        model, ps = model_builder._construct(cfg.model, True, 0)
        assert type(model) is frcnn.FasterRCNNMetaArch and len(ps.specs) == n_vars
        by = {s.name: s for s in ps.specs}
        assert by["SecondStageBoxPredictor/FC_0_%d/weights" % fc_out].shape == (fc_in, fc_out)
        assert ("SecondStageBoxPredictor/FC_1_%d/weights" % fc_out in by) == (n_fc == 2)
        mtl = cfg.model.mtl
        assert mtl.window and mtl.closeness and mtl.edgemask and mtl.refine
        f_lr, mom = trainer.learning_rate_fn(cfg.train_config.optimizer)
        assert f_lr(0) > 0 and mom == 0.9
    full = config.parse_pipeline_config(open(os.path.join(cdir, "frcnn_vgg16_voc_mtl.config")).read()).model.faster_rcnn
    assert int(full.num_classes) == 20 and str(full.feature_extractor.freeze_layer) == "conv2"
    assert (int(full.initial_crop_size), int(full.maxpool_kernel_size), int(full.maxpool_stride)) == (14, 2, 2)


@pytest.mark.parametrize("freeze,training,want", [
    ("", True, [True] * 5), ("conv1", True, [False, True, True, True, True]),
    ("conv3", True, [False, False, False, True, True]), ("conv5", True, [False] * 5),
    ("", False, [False] * 5), ("conv3", False, [False] * 5)])
def test_freeze_layer_table(freeze, training, want):
    from mtl_ssl_amd import model_builder
    specs = model_builder.variable_specs(_cfg("freeze_layer: '%s'" % freeze).model, is_training=training)
    for s in specs[:26]:
        g = int(s.name[len(TRUNK) + 4])
        assert s.trainable == want[g - 1], (s.name, freeze, training)
    # feature_extractor.trainable: false freezes everything
    off = model_builder.variable_specs(_cfg("freeze_layer: '%s' trainable: false" % freeze).model, is_training=training)
    assert not any(s.trainable for s in off[:26])


def test_refusals():
    from mtl_ssl_amd import model_builder, vgg
    for bad in (None, "conv6", "block2", "conv0"):
        fields = "" if bad is None else "freeze_layer: '%s'" % bad           # unset: the proto default 'block1'
        with pytest.raises(ValueError) as e:
            model_builder.variable_specs(_cfg(fields).model, True)
        msg = str(e.value)
        assert all(repr(v) in msg for v in vgg.FREEZE_LAYERS) and "must set" in msg, msg
    assert vgg.FREEZE_LAYERS == ("", "conv1", "conv2", "conv3", "conv4", "conv5")
    with pytest.raises(ValueError, match="no BatchNorm"):
        model_builder.variable_specs(_cfg("freeze_layer: 'conv1' batch_norm_trainable: true").model, True)
    model_builder.variable_specs(_cfg("freeze_layer: 'conv1' batch_norm_trainable: false").model, True)
    with pytest.raises(ValueError, match="must be 8 or 16"):
        model_builder.variable_specs(_cfg("freeze_layer: 'conv1' first_stage_features_stride: 4").model, True)
    assert len(model_builder.variable_specs(_cfg("freeze_layer: 'conv1' first_stage_features_stride: 8").model, True)) \
        == len(model_builder.variable_specs(_cfg().model, True))              # checked, otherwise unused


def test_rfcn_with_the_identity_tower_is_refused():
    from mtl_ssl_amd import config, model_builder
    text = open(os.path.join(ROOT, "configs", "smoke_rfcn_resnet50_mtl.config")).read()
    import re
    text, n = re.subn(r"feature_extractor \{[^}]*\}", "feature_extractor { type: 'faster_rcnn_vgg_16' freeze_layer: 'conv1' }",
                      text, count=1)
    assert n == 1
    with pytest.raises(ValueError, match="rfcn_box_predictor with feature_extractor FasterRCNNVgg16FeatureExtractor"):
        model_builder.variable_specs(config.parse_pipeline_config(text).model, True)


def test_tower_output_mask_follows_the_towers_activation():
    """The predictors' backward masks by the tower's output only when that output is an activation of the tower."""
    from mtl_ssl_amd import mobilenet, resnet, vgg
    feat = object()
    assert vgg.IdentityTower(512).out_mask(feat) == dict(mask_ref=None, mask6=False)
    assert resnet.BoxClassifierTower.out_mask(feat) == dict(mask_ref=feat, mask6=False)
    assert mobilenet.MobilenetTower.out_mask(feat) == dict(mask_ref=feat, mask6=True)
    t = vgg.IdentityTower(512)
    assert t.layers() == [] and t.out_hw(7) == (7, 7) and t.cout == 512
    x = torch.zeros(2, 7, 7, 512)
    assert t.forward(x, True) == (x, None) and t.backward(x, x, None, True, masked=True) is x


def test_classification_checkpoint_round_trip(tmp_path):
    """slim's vgg_16.ckpt names: the scope is stripped; fc6 / fc7 / fc8 of such a checkpoint match no variable."""
    from mtl_ssl_amd import checkpoint, config, model_builder, tf_checkpoint
    prefix = str(tmp_path / "vgg_16.ckpt")
    text = open(SMOKE).read().replace("train_config {", "train_config {\n  fine_tune_checkpoint: '%s'\n"
                                      "  from_detection_checkpoint: false" % prefix, 1)
    cfg = config.parse_pipeline_config(text)
    model, ps = model_builder._construct(cfg.model, True, 0)
    ps.finalize("cpu", seed=0)
    vm = checkpoint.classification_checkpoint_map(ps, [checkpoint.SCOPES["first_stage_fe"], checkpoint.SCOPES["second_stage_fe"]])
    assert sorted(vm) == sorted(n[len("FirstStageFeatureExtractor/"):] for n, _ in vgg_ref.trunk_names())
    assert vm["vgg_16/conv3/conv3_2/weights"] == TRUNK + "conv3/conv3_2/weights"
    assert vm["vgg_16/conv1/conv1_1/biases"] == TRUNK + "conv1/conv1_1/biases"
    rng = np.random.RandomState(5)
    src = {ck: rng.standard_normal(ps.by_name[name].shape).astype(np.float32) for ck, name in vm.items()}
    src["vgg_16/fc6/weights"] = rng.standard_normal((7, 7, 512, 8)).astype(np.float32)
    src["vgg_16/fc6/biases"] = np.ones((8,), np.float32)
    src["global_step"] = np.asarray(0, np.int64)
    tf_checkpoint.write_bundle(prefix, src)
    before = ps.state_dict()
    ck = checkpoint.open_checkpoint(str(cfg.train_config.fine_tune_checkpoint))
    done = checkpoint.init_from_checkpoint(model, ck, cfg.train_config, cfg.model.mtl)      # aux tower maps: empty sets
    assert sorted(done) == sorted(vm.values()) and len(done) == 26
    after = ps.state_dict()
    for ckn, name in vm.items():
        assert np.array_equal(after[name], src[ckn]), name
    for name in after:
        if name not in done:
            assert np.array_equal(after[name], before[name]), name
    # a detection checkpoint restores the same 26 under their own names
    assert sorted(checkpoint.restore_map(ps, True)) == sorted(vm.values())
    # share_second_stage_init: the aux scopes hold predictors only — no tower copy to initialise, nothing a
    # classification checkpoint names
    maps = checkpoint.mtl_init_maps(ps, cfg.model.mtl, False, True)
    assert len(maps) == 3 and not [k for m in maps for k in m if "vgg_16" in k or k in src]


def test_export_writes_and_reads_back_the_variable_list(tmp_path):
    from mtl_ssl_amd import config, model_builder, tf_checkpoint
    specs = model_builder.variable_specs(config.parse_pipeline_config(open(SMOKE).read()).model, is_training=False)
    rng = np.random.RandomState(3)
    src = {}
    for s in specs:
        src[s.name] = rng.standard_normal(s.shape).astype(np.float32)
        src[s.name + "/Momentum"] = src[s.name] * 0.5
    src["global_step"] = np.asarray(3, np.int64)
    p = str(tmp_path / "model.ckpt.npz")
    np.savez(p, **src)
    out = str(tmp_path / "exported")
    r = subprocess.run([sys.executable, "-m", "mtl_ssl_amd.export_inference_graph", "--input_type", "image_tensor",
                        "--pipeline_config_path", SMOKE, "--trained_checkpoint_prefix", p[:-len(".npz")],
                        "--output_directory", out], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = tf_checkpoint.open_tf_checkpoint(os.path.join(out, "model.ckpt"), verify=True)
    assert sorted(got.keys()) == sorted(s.name for s in specs)
    assert all(np.array_equal(got[s.name], src[s.name]) for s in specs)
    assert json.load(open(os.path.join(out, "export.json")))["num_variables"] == len(specs) == 50


def _oracle(values, dtype=np.float64):
    return vgg_ref.VggOracle({"arch": "vgg_16"}, values, dtype)


def test_oracle_trunk_geometry_in_float64():
    rng = np.random.RandomState(0)
    values = {}
    for name, shape in vgg_ref.trunk_names():
        values[name] = (rng.standard_normal(shape) * (0.1 if len(shape) == 4 else 0.01)).astype(np.float32)
    img = torch.as_tensor(rng.uniform(0, 255, (1, 35, 37, 3)))
    o = _oracle(values)
    y = o.trunk_from_rgb(img).detach()
    assert tuple(y.shape) == (1, 2, 2, 512) and y.dtype == torch.float64       # 35->17->8->4->2, 37->18->9->4->2
    assert float(y.min()) >= 0.0
    # Oracle.step hands the trunk img - MEANS: the same map comes out
    from oracle.model import MEANS
    y2 = o.trunk(img - torch.tensor(MEANS)).detach()
    assert float((y - y2).abs().max()) <= 1e-9 * float(y.abs().max())
    # preprocessing: channel flip, Caffe's means per BGR channel
    px = o.preprocess(torch.tensor([[[[10.0, 20.0, 30.0]]]], dtype=torch.float64))
    np.testing.assert_allclose(px.numpy().ravel(), [30 - np.float32(102.9801), 20 - np.float32(115.9465),
                                                    10 - np.float32(122.7717)], rtol=0, atol=1e-12)


def test_oracle_valid_pool_drops_the_last_row():
    """One-channel pattern through conv1_1 (identity tap, channel 0 of BGR = blue), conv1_2 (identity) and pool1 on a
    5x4 image: the VALID 2x2 / 2 pool gives 2x2 and never sees row 4, which holds the largest values."""
    values = {n: np.zeros(s, np.float32) for n, s in vgg_ref.trunk_names()}
    values[TRUNK + "conv1/conv1_1/weights"][1, 1, 0, 0] = 1.0                  # centre tap, BGR channel 0 -> channel 0
    values[TRUNK + "conv1/conv1_2/weights"][1, 1, 0, 0] = 1.0
    o = _oracle(values)
    blue = np.arange(20, dtype=np.float64).reshape(5, 4) * 10.0 + 110.0        # all above the blue mean 102.9801
    img = np.zeros((1, 5, 4, 3))
    img[0, :, :, 2] = blue                                                      # RGB: blue is the last channel
    x = o.preprocess(torch.as_tensor(img))
    for i in (1, 2):
        s = TRUNK + "conv1/conv1_%d" % i
        x = torch.relu(vgg_ref.T.conv2d(x, o.v[s + "/weights"], 1, 1, "SAME") + o.v[s + "/biases"])
    x = x.detach()
    pooled = vgg_ref.T.max_pool(x, 2, 2, "VALID")
    assert tuple(pooled.shape) == (1, 2, 2, 64)
    want = (blue - np.float32(102.9801))[[1, 1, 3, 3], [1, 3, 1, 3]].reshape(2, 2)       # max of each 2x2 window
    np.testing.assert_allclose(pooled[0, :, :, 0].numpy(), want, rtol=0, atol=1e-9)
    assert float(pooled.max()) < float(x[0, 4].max())                           # row 4 was dropped
    assert float(pooled[..., 1:].abs().max()) == 0.0
