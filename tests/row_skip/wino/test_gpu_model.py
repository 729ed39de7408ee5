"""Row-group activity at model level with the 3x3 layers included: one training step of the smoke configuration with
the switch on against off — losses, the flat gradient buffer and the updated weights agree bit for bit — after checking
that the closeness tower's 3x3 layers run on a Winograd plan there, i.e. that the step went through the packed path
(test_gpu_winograd.py beside this file is the kernel-level half)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import ops
    assert torch.cuda.is_available()
    return ops


def _one_step(ops, skip):
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", "smoke_resnet50_mtl.config")).read())
    r = cfg.model.faster_rcnn.image_resizer.keep_aspect_ratio_resizer
    H, W, K = int(r.min_dimension), int(r.max_dimension), int(cfg.model.faster_rcnn.num_classes)
    ops.set_row_skip(skip)
    try:
        model = model_builder.build(cfg.model, True, "cuda:0", seed=1)
        tr = trainer.Trainer(model, cfg.train_config, 1)
        batch = synthetic.make_batch(2, H, W, K, seed=5, device="cuda:0", max_gt=4, num_windows=6)
        losses = tr.forward_backward(batch)
        torch.cuda.synchronize()
        losses = {k: v.clone() for k, v in losses.items()}
        grads, active = model.ps.grads.clone(), tr._pd["_clo_active"].clone()
        tr.apply_gradients()
        torch.cuda.synchronize()
        plans = [(ops.conv_plan_info(d, mode)["family"], d.N, d.H * d.W)
                 for l in model.closeness_tower.layers() if getattr(l, "k", 0) == 3
                 for d in l._desc.values() for mode in (1, 2)]
        return grads, model.ps.weights.clone(), losses, active, plans
    finally:
        ops.set_row_skip(1)


def test_training_step_with_winograd_layers_is_bit_identical_with_row_skip_on_and_off(ops):
    g_off, w_off, l_off, a_off, plans = _one_step(ops, 0)
    assert plans and all(f.startswith("winograd") for f, _, _ in plans), plans      # the 3x3 layers take the new path
    assert all(n == a_off.numel() for _, n, _ in plans), (plans, a_off.numel())     # ... with one flag per batch entry
    assert 0 < int(a_off.sum()) < a_off.numel(), "the batch must hold an active and an inactive RoI"
    g_on, w_on, l_on, a_on, _ = _one_step(ops, 1)
    assert torch.equal(a_on, a_off)
    assert set(l_on) == set(l_off) and "closeness_classification_loss" in l_on
    for k in l_off:
        assert torch.equal(l_on[k], l_off[k]), k
    assert torch.isfinite(g_off).all() and g_off.abs().max() > 0
    assert torch.equal(g_on, g_off)
    assert torch.isfinite(w_off).all() and torch.equal(w_on, w_off)
