"""The float32 matmul precision keyword through the whole model: Trainer(..., float32_matmul_precision=...) and
Detector(..., float32_matmul_precision=...) on a variant of the smoke configuration with 512 RoIs per image (25 088 rows
of 7 x 7 RoI map: enough 256 x 256 tiles for the towers' wide 1x1 layers to run on the split engine directly, and for
their 3x3 layers' Winograd-domain GEMM stacks to run on it with six products — the whole-7-span variant has one
Winograd tile per RoI and 81 planes of 2 filter tiles, so it needs more than 256 RoIs to reach 192 tiles).

No whole-model numeric bound is asserted (none can be derived); what is asserted is which engines ran
(ops.engine_launches), finiteness, re-run determinism, and that leaving the keyword out changes nothing."""
import os

import numpy as np
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
    prev = ops.get_float32_matmul_precision()
    ops.set_float32_matmul_precision("highest")          # the process at its default
    yield ops
    ops.set_float32_matmul_precision(prev)


def _config_text():
    text = open(os.path.join(ROOT, "configs", "smoke_resnet50_mtl.config")).read()
    for old, new in (("first_stage_max_proposals: 40", "first_stage_max_proposals: 512"),
                     ("second_stage_batch_size: 16", "second_stage_batch_size: 512")):
        assert text.count(old) == 1
        text = text.replace(old, new)
    return text


def _one_step(ops, precision):
    """One forward + backward of a freshly built model (same seed, same batch) -> gradients, losses, launches."""
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(_config_text())
    r = cfg.model.faster_rcnn.image_resizer.keep_aspect_ratio_resizer
    H, W, K = int(r.min_dimension), int(r.max_dimension), int(cfg.model.faster_rcnn.num_classes)
    try:
        model = model_builder.build(cfg.model, True, "cuda:0", seed=1)
        tr = trainer.Trainer(model, cfg.train_config, 1, float32_matmul_precision=precision)
        level = ops.get_float32_matmul_precision()
        batch = synthetic.make_batch(1, H, W, K, seed=5, device="cuda:0", max_gt=4, num_windows=6)
        ops.engine_launches(reset=True)
        losses = tr.forward_backward(batch)
        torch.cuda.synchronize()
        counts = ops.engine_launches(reset=True)
        return model.ps.grads.clone(), {k: v.clone() for k, v in losses.items()}, counts, level
    finally:
        ops.set_float32_matmul_precision("highest")


@pytest.fixture(scope="module")
def steps(ops):
    """Each step once, shared by the tests below: `high` twice, the keyword left out, `highest`."""
    return {"high": _one_step(ops, "high"), "high again": _one_step(ops, "high"),
            "none": _one_step(ops, None), "highest": _one_step(ops, "highest")}


def test_trainer_keyword_selects_the_engines(steps):
    grads, losses, counts, level = steps["high"]
    assert level == "high"
    # both > 0: a configuration that stops qualifying fails here instead of passing vacuously
    assert counts["three"] > 0 and counts["six"] > 0, counts
    assert counts["one"] == 0 and counts["native"] > 0, counts
    assert losses and all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0


def test_a_second_identical_step_is_bit_identical(steps):
    (g0, l0, c0, _), (g1, l1, c1, _) = steps["high"], steps["high again"]
    assert c0 == c1 and set(l0) == set(l1)
    for k in l0:
        assert torch.equal(l0[k], l1[k]), k
    assert torch.equal(g0, g1)


def test_keyword_left_out_is_the_default_bit_for_bit(steps):
    (g0, l0, c0, lv0), (g1, l1, c1, lv1) = steps["none"], steps["highest"]
    assert lv0 == lv1 == "highest"
    for c in (c0, c1):
        assert c["native"] > 0 and c["six"] == c["three"] == c["one"] == 0, c
    assert c0 == c1 and set(l0) == set(l1)
    for k in l0:
        assert torch.equal(l0[k], l1[k]), k
    assert torch.equal(g0, g1)
    assert not torch.equal(g0, steps["high"][0])          # and `high` did compute something else


def test_detector_keyword_selects_the_engines(ops, tmp_path):
    from mtl_ssl_amd import config, inference, model_builder, params
    text = _config_text()
    cfgp = str(tmp_path / "pipeline.config")
    open(cfgp, "w").write(text)
    cfg = config.parse_pipeline_config(text)
    state = {"global_step": np.asarray(1, np.int64)}
    for s in model_builder.variable_specs(cfg.model, is_training=False):
        state[s.name] = params.init_value(s, 1)
        state[s.name + "/Momentum"] = np.zeros(s.shape, np.float32)
    np.savez(str(tmp_path / "model.ckpt.npz"), **state)
    rng = np.random.RandomState(3)
    y, x = np.mgrid[0:160, 0:224].astype(np.float32)
    base = np.stack([x / 224 * 255, y / 160 * 255, (x + y) / 384 * 255], -1)
    picture = np.clip(base + rng.normal(0, 25, base.shape), 0, 255).astype(np.uint8)
    try:
        det = inference.Detector(cfgp, str(tmp_path / "model.ckpt"), float32_matmul_precision="medium")
        assert ops.get_float32_matmul_precision() == "medium"
        ops.engine_launches(reset=True)
        out = det.detect_images([picture])[0]
        torch.cuda.synchronize()
        counts = ops.engine_launches(reset=True)
        assert counts["one"] > 0 and counts["six"] > 0 and counts["three"] == 0 and counts["native"] > 0, counts
        assert np.isfinite(out["detection_scores"]).all() and np.isfinite(out["detection_boxes"]).all()
    finally:
        ops.set_float32_matmul_precision("highest")
