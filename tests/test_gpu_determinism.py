"""Run-to-run bit-identity of a whole training step's losses and gradients, every architecture family.

No kernel on the gradient path adds floats in an order that depends on timing: the RoI-crop backward accumulates in
64-bit fixed point in LDS, the PS-RoI, bilinear-resize and overlapping max-pool backwards are gathers, split-K partial
products are folded in slice order. Same weights + same batch + same step counter must therefore give the same bits.
(The first evaluation of a problem shape that is not in conv_plans.json times tile candidates and keeps the last
candidate's output — another summation order — so identity is asserted between evaluations two and three.)"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cfg_name", ["smoke_resnet50_mtl.config", "smoke_rfcn_resnet50_mtl.config",
                                      "smoke_mobilenet_v1_mtl.config", "smoke_inception_resnet_v2_mtl.config"])
def test_step_is_bit_reproducible(cfg_name):
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", cfg_name)).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    model = model_builder.build(cfg.model, True, "cuda", seed=5)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    batch = tr.stage_batch(synthetic.make_batch(2, 160, 224, K, seed=21, device="cuda", max_gt=4, num_windows=6))
    tr.forward_backward(batch)
    torch.cuda.synchronize()
    l2 = {k: float(v.item()) for k, v in tr.forward_backward(batch).items()}
    torch.cuda.synchronize()
    g2 = model.ps.grads.clone()
    assert float(g2.abs().sum()) > 0
    l3 = {k: float(v.item()) for k, v in tr.forward_backward(batch).items()}
    torch.cuda.synchronize()
    assert l3 == l2
    assert torch.equal(model.ps.grads, g2), float((model.ps.grads - g2).norm() / g2.norm())


@pytest.mark.parametrize("cfg_name", ["smoke_resnet50_mtl.config", "smoke_rfcn_resnet50_mtl.config",
                                      "smoke_inception_resnet_v2_mtl.config"])
def test_update_with_fused_fold_equals_update_then_fold(cfg_name, monkeypatch):
    """mtlssl_sgd_momentum_clip_fold refreshes the shadow weights in the optimizer launch when no SCALE vector trains —
    every BatchNorm frozen (ResNet), or a normaliser without gamma whose beta alone trains (Inception-ResNet-v2's
    slim.batch_norm(scale=False): the folded scale is 1/sqrt(var + eps), beta only moves the shift; the residual `up`
    convolutions fold a constant): weights, momentum accumulators and shadow weights after three steps are bit-identical
    to the two-launch form (mtlssl_sgd_momentum_clip, then mtlssl_fold_scales)."""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", cfg_name)).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    state = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MTLSSL_FUSE_FOLD", mode)
        model = model_builder.build(cfg.model, True, "cuda", seed=5)
        tr = trainer.Trainer(model, cfg.train_config, 1)
        assert tr.fuse_fold == (mode == "1")
        batch = tr.stage_batch(synthetic.make_batch(2, 160, 224, K, seed=21, device="cuda", max_gt=4, num_windows=6))
        tr.step(batch)               # the first evaluation may autotune (another summation order): not compared
        tr.step(batch)
        tr.step(batch)
        torch.cuda.synchronize()
        state[mode] = (model.ps.weights.clone(), model.ps.accum.clone(), model.ps.eff.clone())
        del tr, model
    if not torch.equal(state["1"][0], state["0"][0]):
        pytest.skip("the two runs autotuned different tiles on their first step; nothing to compare bit-wise")
    for a, b in zip(state["1"], state["0"]):
        assert torch.equal(a, b)
    assert float((state["1"][2] - state["1"][0]).abs().max()) > 0     # the shadow weights do differ from the raw ones


@pytest.mark.parametrize("cfg_name", ["smoke_mobilenet_v1_mtl.config"])
def test_fused_fold_is_off_when_batch_norm_parameters_train(cfg_name):
    """MobileNet-v1 trains BatchNorm GAMMA: its scale vectors change with the update, so the fold has to follow the refresh
    of the normaliser constants and stays a launch of its own. (Inception-ResNet-v2 trains beta only — no gamma variable —
    and takes the fused form: test_update_with_fused_fold_equals_update_then_fold.)"""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import config, model_builder, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", cfg_name)).read())
    model = model_builder.build(cfg.model, True, "cuda", seed=5)
    assert any(getattr(l, "bn_trainable", False) and getattr(l, "gamma", None) is not None for l in model.layers)
    assert not trainer.Trainer(model, cfg.train_config, 1).fuse_fold


@pytest.mark.parametrize("cfg_name", ["smoke_resnet50_mtl.config", "smoke_rfcn_resnet50_mtl.config"])
def test_forward_overlap_switches_do_not_change_a_bit(cfg_name, monkeypatch):
    """MTLSSL_CLOSENESS_FWD_SIDE / MTLSSL_REFINE_EARLY (closeness tower beside the main tower; the refiner's window
    pass on the third stream) only move launches between streams. Off by default since round 5 (chains of chip-filling
    GEMMs gain nothing from time-slicing each other: profiles/r05_fwd_overlap_ab.txt); with them on, losses and
    gradients of a step are bit-identical to the serial schedule."""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", cfg_name)).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MTLSSL_CLOSENESS_FWD_SIDE", mode)
        monkeypatch.setenv("MTLSSL_REFINE_EARLY", mode)
        model = model_builder.build(cfg.model, True, "cuda", seed=5)
        if "rfcn" not in cfg_name:
            assert (model._refine_stream() is not None) == (mode == "1")          # the early window pass is (not) taken
        tr = trainer.Trainer(model, cfg.train_config, 1)
        batch = tr.stage_batch(synthetic.make_batch(2, 160, 224, K, seed=21, device="cuda", max_gt=4, num_windows=6))
        tr.forward_backward(batch)
        losses = {k: float(v.item()) for k, v in tr.forward_backward(batch).items()}
        torch.cuda.synchronize()
        res[mode] = (losses, model.ps.grads.clone())
        del tr, model
    assert res["0"][0] == res["1"][0]
    assert torch.equal(res["0"][1], res["1"][1])


@pytest.mark.parametrize("cfg_name,refined_weight", [("smoke_resnet50_mtl.config", None),
                                                     ("smoke_rfcn_resnet50_mtl.config", None),
                                                     ("smoke_resnet50_mtl.config", 0.5)])
def test_split_loss_equals_whole_loss_bit_for_bit(cfg_name, refined_weight, monkeypatch):
    """MTLSSL_SPLIT_LOSS=1 (loss(part="early") on the side stream, the refiner, then loss(part="late")) against
    MTLSSL_SPLIT_LOSS=0 (the refiner, then loss(part="all")): the same terms, the same loss_scale on every gradient,
    so the losses and gradients of a step are bit-identical. With refined_classification_loss_weight 0.5 the refined
    term no longer shares the classification term's scales and computes its own."""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    text = open(os.path.join(ROOT, "configs", cfg_name)).read()
    if refined_weight is not None:
        assert "refined_classification_loss_weight: 1.0" in text
        text = text.replace("refined_classification_loss_weight: 1.0",
                            "refined_classification_loss_weight: %s" % refined_weight)
    cfg = config.parse_pipeline_config(text)
    K = int(cfg.model.faster_rcnn.num_classes)
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MTLSSL_SPLIT_LOSS", mode)
        model = model_builder.build(cfg.model, True, "cuda", seed=5)
        tr = trainer.Trainer(model, cfg.train_config, 1)
        assert tr.split_loss == (mode == "1")
        batch = tr.stage_batch(synthetic.make_batch(2, 160, 224, K, seed=21, device="cuda", max_gt=4, num_windows=6))
        tr.forward_backward(batch)
        losses = {k: float(v.item()) for k, v in tr.forward_backward(batch).items()}
        torch.cuda.synchronize()
        assert "refined_classification_loss" in losses
        res[mode] = (losses, model.ps.grads.clone())
        del tr, model
    assert res["1"][0] == res["0"][0]
    assert torch.equal(res["1"][1], res["0"][1])


@pytest.mark.parametrize("cfg_name", ["smoke_mobilenet_v1_mtl.config", os.path.join("vgg16", "smoke_vgg16_mtl.config")])
def test_extractors_that_ignore_the_wgrad_stream_do_not_change_a_bit_with_it(cfg_name, monkeypatch):
    """MobileNet-v1 and VGG-16 (extractor and tower) take the filter-gradient executor like every family and run their
    filter gradients inline. MTLSSL_WGRAD_STREAM=1 hands them a real nn.WgradStream: every variable's gradient still
    comes from the same launches in the same order — only the three head filter gradients move to the side stream — so
    losses and gradients are bit-identical to the default (inline) schedule: no tolerance."""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import config, model_builder, nn, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", cfg_name)).read())
    K = int(cfg.model.faster_rcnn.num_classes)
    res = {}
    for mode in (None, "1"):
        if mode is None:
            monkeypatch.delenv("MTLSSL_WGRAD_STREAM", raising=False)
        else:
            monkeypatch.setenv("MTLSSL_WGRAD_STREAM", mode)
        model = model_builder.build(cfg.model, True, "cuda", seed=5)
        assert isinstance(model._wgrad_exec(), nn.WgradStream) == (mode == "1")
        tr = trainer.Trainer(model, cfg.train_config, 1)
        batch = tr.stage_batch(synthetic.make_batch(2, 160, 224, K, seed=21, device="cuda", max_gt=4, num_windows=6))
        tr.forward_backward(batch)
        loss_dict = tr.forward_backward(batch)
        losses = {k: float(v.item()) for k, v in loss_dict.items()}
        torch.cuda.synchronize()
        res[mode] = (losses, model.ps.grads.clone())
        del tr, model
    assert float(res[None][1].abs().sum()) > 0
    assert res[None][0].keys() == res["1"][0].keys() and res[None][0] == res["1"][0]
    assert torch.equal(res[None][1], res["1"][1])
