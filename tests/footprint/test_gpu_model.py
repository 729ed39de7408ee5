"""Footprint of whole training steps: every size query in front of the exact call production makes, side streams
included. For each smoke configuration one training step (forward, backward, optimizer update) runs twice from
identical state — once with the ordinary workspace cache, once under GuardedWorkspaces (tests/footprint/guarded.py),
where every workspace is a fresh buffer of exactly the bytes asked for, allocated on the stream current at the call and
kept alive until the check. Asserted: every guard intact; every loss term, the flat gradient buffer and the updated
weights torch.equal between the two runs. Hand-outs and bytes per workspace key go to the parity report."""
import os

import pytest
import torch

from tests import parity_report
from tests.footprint.guarded import GuardedWorkspaces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIGS = ["smoke_resnet50_mtl", "smoke_mobilenet_v1_mtl", "smoke_inception_resnet_v2_mtl", "smoke_rfcn_resnet50_mtl",
           "vgg16/smoke_vgg16_mtl"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()


def _one_step(name):
    """Model, trainer and batch as the sibling whole-step tests build them (tests/test_gpu_mobilenet.py, _inception.py,
    _rfcn.py, tests/vgg/test_gpu_model.py; the ResNet-50 smoke step as __graft_entry__.smoke())."""
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, "configs", name + ".config")).read())
    if name == "smoke_resnet50_mtl":
        r = cfg.model.faster_rcnn.image_resizer.keep_aspect_ratio_resizer
        H, W, K = int(r.min_dimension), int(r.max_dimension), int(cfg.model.faster_rcnn.num_classes)
        model = model_builder.build(cfg.model, True, "cuda:0", seed=1)
        batch = synthetic.make_batch(2, H, W, K, seed=5, device="cuda:0", max_gt=4, num_windows=6)
    else:
        model = model_builder.build(cfg.model, True, "cuda", seed=3)
        batch = synthetic.make_batch(2, 160, 224, 5, seed=11, device="cuda", max_gt=4, num_windows=6)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    losses = tr.forward_backward(batch)
    torch.cuda.synchronize()
    losses = {k: v.clone() for k, v in losses.items()}
    grads = model.ps.grads.clone()
    tr.apply_gradients()
    torch.cuda.synchronize()
    return losses, grads, model.ps.weights.clone()


@pytest.mark.parametrize("name", CONFIGS)
def test_training_step_is_bit_identical_inside_exact_workspaces(name):
    l0, g0, w0 = _one_step(name)
    with GuardedWorkspaces() as gw:
        l1, g1, w1 = _one_step(name)
    gw.check()
    assert gw.handouts, "the step asked for no workspace at all"
    assert set(l0) == set(l1) and l0
    for k in l0:
        assert torch.equal(l0[k], l1[k]), (name, k, float(l0[k]), float(l1[k]))
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert torch.equal(g0, g1), (name, "gradients")
    assert torch.equal(w0, w1), (name, "updated weights")
    parity_report.add("footprint step %s: %d hand-outs — %s" % (name, len(gw.handouts), gw.report()))
