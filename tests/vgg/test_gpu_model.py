"""The whole Faster R-CNN VGG-16 training step on the smoke configuration against VggOracle, staged like every
model-level test (tests/parity_report.py): RPN floats to 1e-3, the proposal chain bit for bit on the device's RPN floats,
losses and gradients on identical boxes, then the gradients against float64."""
import numpy as np
import pytest
import torch

from tests import parity_report
from tests.vgg import vgg_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()


def _step(extra_mtl=""):
    from mtl_ssl_amd import model_builder, synthetic, trainer, vgg
    cfg = vgg_ref.smoke_config(extra_mtl)
    model = model_builder.build(cfg.model, True, "cuda", seed=3)
    assert isinstance(model._feature_extractor, vgg.FasterRCNNVgg16FeatureExtractor)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    batch = synthetic.make_batch(2, 160, 224, 5, seed=11, device="cuda", max_gt=4, num_windows=6)
    values = model.ps.state_dict()
    reports = {}
    model.ps.grad_ready_hook = lambda sp: reports.__setitem__(sp.name, reports.get(sp.name, 0) + 1)
    losses = tr.forward_backward(batch)
    model.ps.grad_ready_hook = None
    torch.cuda.synchronize()
    # every trainable variable reports "gradient final" exactly once per step
    assert reports == {sp.name: 1 for sp in model.ps.trainable_specs}, \
        sorted(set(reports) ^ {sp.name for sp in model.ps.trainable_specs})[:5]
    got = {k: float(v.item()) for k, v in losses.items()}
    hb = dict(batch)
    hb["images"] = batch["images"].cpu().numpy()
    return cfg, model, tr, batch, values, got, hb


def _losses_agree(tag, got, ref):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = 0.0
    for k in sorted(ref):
        err = abs(got[k] - ref[k]) / max(abs(ref[k]), 1e-3)
        worst = max(worst, err)
        print("    %s %s: device %.7g oracle %.7g rel err %.2e" % (tag, k, got[k], ref[k], err))
        assert err <= 1e-3, (tag, k, got[k], ref[k])
    parity_report.add("    %s: %d losses, worst rel err %.2e" % (tag, len(ref), worst))


def test_vgg16_step_matches_oracle_and_float64():
    cfg, model, tr, batch, values, got, hb = _step()
    mtl = cfg.model.mtl
    assert mtl.window and mtl.closeness and mtl.edgemask and mtl.refine
    assert not [n for n in model.ps.by_name if n.startswith("SecondStageFeatureExtractor")]
    hp = vgg_ref.hyper_params(cfg)
    pd = tr._pd
    ref, rgrads, aux = parity_report.oracle_on_device_rpn(vgg_ref.VggOracle, hp, values, hb, model.seed, 0, pd)
    feat_err = float(np.abs(pd["rpn_features_to_crop"].cpu().numpy() - aux["features"]).max() / np.abs(aux["features"]).max())
    assert feat_err < 1e-3, feat_err
    np.testing.assert_array_equal(pd["_rpn_targets"]["match"].cpu().numpy(), aux["rpn_match"])
    _losses_agree("Faster R-CNN VGG-16 160x224", got, ref)
    grads = model.ps.grads_dict()
    assert not [n for n in grads if "/conv1/" in n] and "FirstStageFeatureExtractor/vgg_16/conv2/conv2_1/weights" in grads
    assert all(n in rgrads for n in grads)
    l2 = parity_report.gradients("Faster R-CNN VGG-16 160x224", grads, rgrads, got, ref)
    assert len(l2) == len(grads) == 46
    parity_report.against_float64("Faster R-CNN VGG-16 160x224", vgg_ref.VggOracle, hp, values, hb, model.seed, 0,
                                  pd["proposal_boxes"].cpu().numpy(), pd["num_proposals"].cpu().numpy(), grads,
                                  feat=pd["rpn_features_to_crop"].cpu().numpy(), d_feat=pd["_gpF"].cpu().numpy())


@pytest.mark.parametrize("extra", ["stop_gradient_for_aux_tasks: false shared_feature: 'classifier_feature_maps'",
                                   "stop_gradient_for_aux_tasks: true"], ids=["shared_classifier_maps", "stop_gradient"])
def test_vgg16_variants_losses_match_oracle(extra):
    """shared_feature 'classifier_feature_maps' makes the "shared tower" the same identity; stop_gradient_for_aux_tasks
    cuts the aux heads off the crops. Losses only."""
    cfg, model, tr, batch, values, got, hb = _step(extra)
    if "shared_feature" in extra:
        assert model.window_tower is model.tower and model.closeness_tower is None
    ref, _, _ = parity_report.oracle_on_device_rpn(vgg_ref.VggOracle, vgg_ref.hyper_params(cfg), values, hb, model.seed, 0, tr._pd)
    _losses_agree("Faster R-CNN VGG-16 160x224 (%s)" % extra.split(":")[-2].split()[-1], got, ref)
    assert np.isfinite(model.ps.grads.sum().item())


def test_a_second_run_of_the_step_gives_the_same_weights():
    from mtl_ssl_amd import model_builder, synthetic, trainer
    cfg = vgg_ref.smoke_config()
    batch = synthetic.make_batch(2, 160, 224, 5, seed=11, device="cuda", max_gt=4, num_windows=6)
    out = []
    for _ in range(2):
        model = model_builder.build(cfg.model, True, "cuda", seed=3)
        tr = trainer.Trainer(model, cfg.train_config, 1)
        before = model.ps.weights.clone()
        tr.step(batch)
        tr.step(batch)
        torch.cuda.synchronize()
        assert not torch.equal(before, model.ps.weights) and bool(torch.isfinite(model.ps.weights).all())
        out.append(model.ps.weights.clone())
    assert torch.equal(out[0], out[1])
