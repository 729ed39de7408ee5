"""Row-group activity at model level: one training step of the smoke configuration with the closeness tower's backward
leaving its zero-scale RoIs out of the 1x1 GEMMs (mtlssl_conv2d_set_row_skip(1), the default) against one that multiplies
every row (0): the flat gradient buffer and every loss must agree bit for bit (the kernel-level half is test_gpu_conv_ops.py
beside this file)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
        return model.ps.grads.clone(), {k: v.clone() for k, v in losses.items()}, tr._pd["_clo_active"].clone()
    finally:
        ops.set_row_skip(1)


def test_training_step_is_bit_identical_with_row_skip_on_and_off(ops):
    g_off, l_off, a_off = _one_step(ops, 0)          # the reference behaviour: every row multiplied
    assert 0 < int(a_off.sum()) < a_off.numel(), "the batch must hold an active and an inactive RoI"
    g_on, l_on, a_on = _one_step(ops, 1)
    assert torch.equal(a_on, a_off)
    assert set(l_on) == set(l_off) and "closeness_classification_loss" in l_on
    for k in l_off:
        assert torch.equal(l_on[k], l_off[k]), k
    assert torch.isfinite(g_off).all() and g_off.abs().max() > 0
    assert torch.equal(g_on, g_off)
