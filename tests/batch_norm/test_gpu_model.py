"""The heads' batch-statistics BatchNorm inside the model: one training step of configs/batch_norm/
smoke_resnet50_bn_mtl.config at 160x224 (batch 2: 140 RPN rows, 32 RoI rows), wired to the kernels that
test_gpu_head_kernels.py checks against float64."""
import os

import numpy as np
import pytest
import torch

from tests.batch_norm import batchnorm_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONFIG = os.path.join(ROOT, "configs", "batch_norm", "smoke_resnet50_bn_mtl.config")
H, W, K = 160, 224, 5
RPN, FC, BOX, CLS = ("FirstStageBoxPredictor/Conv", "SecondStageBoxPredictor/FC_0_64",
                     "SecondStageBoxPredictor/BoxEncodingPredictor", "SecondStageBoxPredictor/ClassPredictor")


def _losses(d):
    return {k: float(v.item()) for k, v in d.items()}


def _norm_layers(model):
    """{scope: (layer, what its forward kept: z, mean, inv_std)} of the last predict_for_training."""
    bp = model.box_predictor
    return {RPN: model.rpn_conv, FC: bp.stack.layers[0], BOX: bp.box, CLS: bp.cls}


def _kept(model, pd):
    bp = pd["_bp"]
    return {RPN: pd["_rpn_norm"], FC: bp["_stack_ctx"][0][3], BOX: bp["_norm_box"], CLS: bp["_norm_class"]}


@pytest.fixture(scope="module")
def stepped():
    """One forward + backward (no update) of the training model -> everything the tests read."""
    import __graft_entry__ as g
    g.build()
    from mtl_ssl_amd import config, model_builder, synthetic, trainer
    cfg = config.parse_pipeline_config(open(CONFIG).read())
    model = model_builder.build(cfg.model, True, "cuda", seed=1)
    tr = trainer.Trainer(model, cfg.train_config, 1)
    batch = synthetic.make_batch(2, H, W, K, seed=5, device="cuda", max_gt=4, num_windows=6)
    before = model.ps.state_dict()
    losses = _losses(tr.forward_backward(batch))
    torch.cuda.synchronize()
    return dict(cfg=cfg, model=model, tr=tr, batch=batch, before=before, losses=losses, pd=tr._pd,
                after=model.ps.state_dict(), grads=model.ps.grads_dict())


def test_step_is_finite_and_every_gamma_beta_gets_a_gradient(stepped):
    assert len(stepped["losses"]) == 8 and all(np.isfinite(v) for v in stepped["losses"].values()), stepped["losses"]
    names = [n for n in stepped["grads"] if "/BatchNorm/" in n]
    assert sorted(names) == sorted([RPN + "/BatchNorm/beta"] + ["%s/BatchNorm/%s" % (s, v) for s in (FC, BOX, CLS)
                                                                for v in ("beta", "gamma")])
    for n in names:
        g = stepped["grads"][n]
        assert np.isfinite(g).all() and np.any(g != 0), n
    for s in (RPN, FC, BOX, CLS):
        assert np.any(stepped["grads"][s + "/weights"] != 0), s


def test_rpn_layer_is_the_kernel_on_the_bias_free_conv_output(stepped):
    from mtl_ssl_amd import ops
    model, pd = stepped["model"], stepped["pd"]
    l, F = model.rpn_conv, pd["rpn_features_to_crop"]
    assert l.batch_stats and l.b is None and l.activation == "relu"
    z = ops.conv2d_fwd(l.desc(F.shape), F, l._w4(), None, None, 0, xf_cache=model.ps.filter_cache)
    assert torch.equal(z, pd["_rpn_norm"]["z"])
    y, mean, inv_std = ops.batch_norm_train_fwd(z, None, model.ps.value(RPN + "/BatchNorm/beta"), 1e-3, ops.EPI_RELU)
    assert torch.equal(y, pd["rpn_box_predictor_features"])
    assert torch.equal(mean, pd["_rpn_norm"]["mean"]) and torch.equal(inv_std, pd["_rpn_norm"]["inv_std"])


def test_moving_averages_follow_the_update_rule_once_per_training_forward(stepped):
    model, pd, before, after = stepped["model"], stepped["pd"], stepped["before"], stepped["after"]
    f = R.moving_average_factor(0.999)
    kept = _kept(model, pd)
    for scope in (RPN, FC, BOX, CLS):
        k = kept[scope]
        mm0, mv0 = before[scope + "/BatchNorm/moving_mean"], before[scope + "/BatchNorm/moving_variance"]
        assert np.all(mm0 == 0) and np.all(mv0 == 1)                     # slim's initial values
        mean = k["mean"].cpu().numpy()
        assert np.array_equal(after[scope + "/BatchNorm/moving_mean"], R.moving_update_fp32(mm0, mean, f)), scope
        # the variance is not among the saved statistics: the float64 definition on the layer's own input z, inside
        # the kernel bound on var (times Bessel's factor and f) plus the four roundings of the sequence, values near 1
        z = k["z"].cpu().numpy().reshape(-1, mean.shape[0])
        n = z.shape[0]
        _, var, _ = R.stats(z, 1e-3)
        want = R.moving_update(mm0, mv0, mean, var, n, f)[1]
        bound = float(f) * R.forward_bounds(z, None, None, 1e-3)["var"] * n / (n - 1) + 4 * R.U * np.maximum(np.abs(want), 1)
        got = after[scope + "/BatchNorm/moving_variance"]
        assert np.any(got != 1.0) and R.worst_ratio(got, want, bound) <= 1.0, scope
    # gamma / beta and the filters were not touched (no update was applied)
    for n_, v in before.items():
        if not n_.endswith(("moving_mean", "moving_variance")):
            assert np.array_equal(v, after[n_]), n_


def test_predict_and_eval_loss_leave_the_moving_averages_alone(stepped):
    from mtl_ssl_amd import model_builder
    model, batch, cfg = stepped["model"], stepped["batch"], stepped["cfg"]
    snap = model.ps.frozen.clone()
    model.predict(model.preprocess(batch["images"]))
    torch.cuda.synchronize()
    assert torch.equal(snap, model.ps.frozen)
    ev = model_builder.build(cfg.model, False, "cuda", seed=1, values=stepped["after"])
    assert not ev.rpn_conv.batch_stats and ev.rpn_conv.w_eff is not None
    ev.provide_groundtruth(batch["groundtruth_boxes"], batch["groundtruth_classes"], batch.get("groundtruth_closeness"))
    ev.provide_window(batch["window_boxes"], batch["window_classes"])
    ev.provide_edgemask(batch["groundtruth_edgemask"])
    snap = ev.ps.frozen.clone()
    pd = ev.predict(ev.preprocess(batch["images"]))
    ev.predict_with_window(pd)
    ev.predict_edgemask(pd)
    pd = ev.predict_with_mtl_results(pd)
    losses = _losses(ev.eval_loss(pd))
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses.values()), losses
    assert torch.equal(snap, ev.ps.frozen)


def test_batch_statistics_losses_equal_the_frozen_fold_on_the_same_statistics(stepped):
    """The same weights, the same step, the moving statistics set to what the batch-statistics forward saved
    (moving_variance = 1 / inv_std^2 - eps, in float64), every normaliser switched to its frozen mode: the folded
    layers compute conv(x, w * scale) + (beta - mean * scale) where the training path computes
    ((conv(x, w) - mean) * inv_std) * gamma + beta. The two differ by where the affine is rounded: the fold rounds
    w * scale once per filter element and sums K products of it, the training path rounds the sum first — either way
    a handful of roundings, each <= u = 6e-8 relative to |z| * scale + |mean| * scale + |beta| (the fold cancels
    z * scale against mean * scale, so a channel whose mean is several standard deviations from zero loses that
    factor); scale itself carries the rounding of moving_variance to fp32 and of rsqrt (<= 2u). With |mean| / std up
    to ~5 that is a few 1e-7 to 1e-6 of a logit's size, and the losses — smooth in the logits, on the same sampled
    anchors and proposals — follow: 1e-5 relative. Observed on an MI355X: <= 2e-6 on the RPN's and the detector's own
    terms, 7.1e-6 on the refined classification term (the refiner's FC layer reads the class logits of three heads
    and its residual adds them back, so their differences arrive twice). A wrong statistic (a biased / unbiased mix-up
    is 1/(2n) = 1.6e-2 at the 32 RoI rows) misses the tolerance by three orders."""
    from mtl_ssl_amd import config, model_builder, trainer
    cfg, batch, pd = stepped["cfg"], stepped["batch"], stepped["pd"]
    values = dict(stepped["before"])
    for scope, k in _kept(stepped["model"], pd).items():
        inv_std = k["inv_std"].cpu().numpy().astype(np.float64)
        values[scope + "/BatchNorm/moving_mean"] = k["mean"].cpu().numpy()
        values[scope + "/BatchNorm/moving_variance"] = (1.0 / inv_std ** 2 - 1e-3).astype(np.float32)
    model = model_builder.build(cfg.model, True, "cuda", seed=1, values=values)
    for l in _norm_layers(model).values():
        l.norm.batch_stats = False
    model.prepare()                                   # folds the moving statistics into shadow filters
    assert all(l.w_eff is not None and not l.batch_stats for l in _norm_layers(model).values())
    tr = trainer.Trainer(model, cfg.train_config, 1)
    m = tr.model
    m.step = 0
    tr.provide(batch)
    fpd = m.predict_for_training(m.preprocess(batch["images"]))
    fpd = m.predict_with_mtl_results(fpd)
    frozen = _losses(m.loss(fpd))
    torch.cuda.synchronize()
    for k, v in stepped["losses"].items():
        print("%s: batch statistics %.9g, frozen fold %.9g, rel %.2e" % (k, v, frozen[k], abs(v - frozen[k]) / abs(v)))
    for k, v in stepped["losses"].items():
        assert abs(v - frozen[k]) <= 1e-5 * abs(v), (k, v, frozen[k])


def test_detector_runs_on_the_saved_state_and_is_deterministic(stepped, tmp_path):
    from mtl_ssl_amd import checkpoint
    from mtl_ssl_amd.inference import Detector
    model, tr = stepped["model"], stepped["tr"]
    path = str(tmp_path / "model.ckpt.npz")
    checkpoint.save(path, model.ps, tr.global_step, tr)
    saved = np.load(path)
    assert np.array_equal(saved[RPN + "/BatchNorm/moving_mean"], stepped["after"][RPN + "/BatchNorm/moving_mean"])
    det = Detector(CONFIG, path)
    images = np.random.RandomState(3).randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    a, b = det.detect_images(images), det.detect_images(images)
    assert len(a) == 2
    for ra, rb in zip(a, b):
        assert sorted(ra) == sorted(rb)
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
            assert np.isfinite(np.asarray(ra[k], np.float64)).all(), k
