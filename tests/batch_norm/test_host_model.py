"""Hyperparams `batch_norm` on the host: the variables a config with normalised heads registers, their trainability,
the refusals, and that the models of the existing smoke configs are exactly what they were
(tests/golden/smoke_variable_specs.json.gz, written from the commit before the normaliser by
tests/golden/make_smoke_variable_specs.py)."""
import os

import pytest

from tests.golden import make_smoke_variable_specs as M

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BN_CONFIG = "configs/batch_norm/smoke_resnet50_bn_mtl.config"
RPN, FC, BOX, CLS = ("FirstStageBoxPredictor/Conv", "SecondStageBoxPredictor/FC_0_64",
                     "SecondStageBoxPredictor/BoxEncodingPredictor", "SecondStageBoxPredictor/ClassPredictor")


def _text(path=BN_CONFIG):
    return open(os.path.join(ROOT, path)).read()


def _specs(text, is_training):
    from mtl_ssl_amd import config, model_builder
    return model_builder.variable_specs(config.parse_pipeline_config(text).model, is_training)


def _by_name(specs):
    return {s.name: s for s in specs}


def test_normalised_layers_have_batch_norm_variables_and_no_biases():
    v = _by_name(_specs(_text(), True))
    for scope, width, scale in ((RPN, 512, False), (FC, 64, True), (BOX, 20, True), (CLS, 6, True)):
        assert scope + "/weights" in v and scope + "/biases" not in v, scope
        for name, init in (("beta", ("zeros",)), ("moving_mean", ("zeros",)), ("moving_variance", ("const", 1.0))):
            s = v["%s/BatchNorm/%s" % (scope, name)]
            assert s.shape == (width,) and tuple(s.init) == init and s.weight_decay == 0.0, s.name
        assert (scope + "/BatchNorm/gamma" in v) == scale, scope           # gamma only where scale: true
        if scale:
            assert tuple(v[scope + "/BatchNorm/gamma"].init) == ("const", 1.0)
    # the two RPN heads run with normalizer_fn=None; the auxiliary predictors and the refiner carry no block
    for scope in ("FirstStageBoxPredictor/BoxEncodingPredictor", "FirstStageBoxPredictor/ClassPredictor",
                  "WindowBoxPredictor/ClassPredictor", "ClosenessBoxPredictor/ClassPredictor", "MTLClassRefiner/fc1"):
        assert scope + "/biases" in v and not any(n.startswith(scope + "/BatchNorm/") for n in v), scope
    # everything else is smoke_resnet50_mtl's model
    plain = _by_name(_specs(_text("configs/smoke_resnet50_mtl.config"), True))
    touched = (RPN, FC, BOX, CLS)
    assert {n for n in v if not n.startswith(touched)} == {n for n in plain if not n.startswith(touched)}


@pytest.mark.parametrize("is_training", [True, False], ids=["train", "inference"])
def test_trainability(is_training):
    v = _by_name(_specs(_text(), is_training))
    for n, s in v.items():
        if "/BatchNorm/" in n and n.startswith((RPN, FC, BOX, CLS)):
            moving = n.endswith(("moving_mean", "moving_variance"))
            assert s.trainable == (is_training and not moving), n
    assert sorted(v) == sorted(_by_name(_specs(_text(), not is_training)))      # the same names in both modes


def test_train_false_keeps_gamma_beta_trainable():
    text = _text().replace("batch_norm { }", "batch_norm { train: false }")
    v = _by_name(_specs(text, True))
    assert v[RPN + "/BatchNorm/beta"].trainable and not v[RPN + "/BatchNorm/moving_mean"].trainable
    from mtl_ssl_amd import config, model_builder
    model, _ = model_builder._construct(config.parse_pipeline_config(text).model, True, 0)
    assert not model.rpn_conv.batch_stats and model.rpn_conv.norm.bn_trainable
    assert model.box_predictor.cls.batch_stats


def test_frozen_rpn_filter_keeps_its_normaliser_trainable():
    text = _text().replace("first_stage_nms_score_threshold", "first_stage_box_predictor_trainable: false "
                           "first_stage_nms_score_threshold")
    v = _by_name(_specs(text, True))
    assert not v[RPN + "/weights"].trainable
    assert v[RPN + "/BatchNorm/beta"].trainable and not v[RPN + "/BatchNorm/moving_variance"].trainable
    from mtl_ssl_amd import config, model_builder
    model, _ = model_builder._construct(config.parse_pipeline_config(text).model, True, 0)
    assert model.rpn_conv.grad_vars() == (model.rpn_conv.norm.beta,)


def test_a_block_without_op_fc_adds_nothing():
    plain = _text("configs/smoke_resnet50_mtl.config")
    block = "fc_hyperparams { op: FC initializer { variance_scaling_initializer"
    assert plain.count(block) == 1
    for op in ("op: CONV", ""):
        text = plain.replace(block, "fc_hyperparams { %s batch_norm { scale: true } initializer "
                                    "{ variance_scaling_initializer" % op)
        for is_training in (True, False):
            assert M.spec_lines(_specs(text, is_training)) == M.spec_lines(_specs(plain, is_training))


REFUSED = {
    "mtl.window_box_predictor": ("window_box_predictor { mask_rcnn_box_predictor { spatial_average: true\n"
                                 "      fc_hyperparams { op: FC "),
    "mtl.closeness_box_predictor": ("closeness_box_predictor { mask_rcnn_box_predictor { spatial_average: true\n"
                                    "      fc_hyperparams { op: FC "),
    "mtl.edgemask_predictor.conv_hyperparams": "conv_hyperparams { op: CONV ",
    "mtl.refiner_fc_hyperparams": "refiner_fc_hyperparams { op: FC ",
}


@pytest.mark.parametrize("field", sorted(REFUSED))
@pytest.mark.parametrize("is_training", [True, False], ids=["train", "inference"])
def test_refused_fields_raise_and_name_the_field(field, is_training):
    text = _text()
    anchor = REFUSED[field]
    assert text.count(anchor) == 1, field
    with pytest.raises(ValueError) as e:
        _specs(text.replace(anchor, anchor + "batch_norm { } "), is_training)
    assert field in str(e.value) and "batch statistics are not built" in str(e.value)


def test_rfcn_and_mobilenet_keep_their_refusals():
    text = _text("configs/smoke_rfcn_resnet50_mtl.config")
    assert "conv_hyperparams {" in text
    from mtl_ssl_amd import config, model_builder
    cfg = config.parse_pipeline_config(text)
    cfg.model.faster_rcnn.second_stage_box_predictor.rfcn_box_predictor.conv_hyperparams["batch_norm"] = \
        config.Msg("BatchNorm")
    with pytest.raises(ValueError, match="rfcn_box_predictor with batch_norm"):
        model_builder.variable_specs(cfg.model, True)
    cfg = config.parse_pipeline_config(_text("configs/smoke_mobilenet_v1_mtl.config"))
    cfg.model.faster_rcnn.feature_extractor["batch_norm_trainable"] = True
    with pytest.raises(ValueError, match="batch_norm_trainable"):
        model_builder.variable_specs(cfg.model, True)


def test_proto_defaults_of_the_block():
    from mtl_ssl_amd import config
    bn = config.parse_pipeline_config(_text()).model.faster_rcnn.first_stage_box_predictor_conv_hyperparams.batch_norm
    assert (bn.decay, bn.center, bn.scale, bn.epsilon, bn.train) == (0.999, True, False, 0.001, True)


def test_existing_smoke_configs_build_the_models_they_built_before():
    golden = M.load_golden()
    configs = M.smoke_configs(ROOT)
    assert len(configs) == 5 and sorted(golden) == sorted("%s:%s" % (c, m) for c in configs for m in ("train", "inference"))
    for key, want in golden.items():
        path, mode = key.split(":")
        assert M.spec_lines(_specs(_text(path), mode == "train")) == want, key


def test_checkpoint_maps_see_the_normaliser_variables():
    """restore_map is built from the ParamStore's names: with restore_box_predictor a detection checkpoint restores the
    heads' BatchNorm/* with their scopes (moving statistics included), a classification checkpoint none of them."""
    from mtl_ssl_amd import checkpoint, config, model_builder
    _, ps = model_builder._construct(config.parse_pipeline_config(_text()).model, True, 0)
    bn = {s.name for s in ps.specs if "/BatchNorm/" in s.name and s.name.startswith((RPN, FC, BOX, CLS))}
    assert len(bn) == 3 + 3 * 4
    assert bn <= set(checkpoint.restore_map(ps, True, restore_box_predictor=True).values())
    assert not bn & set(checkpoint.restore_map(ps, True).values())
    assert not bn & set(checkpoint.restore_map(ps, False).values())
