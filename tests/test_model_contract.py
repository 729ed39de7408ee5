"""The layer / tower / extractor contract of nn.py, on the host: every shipped config builds a model
whose parts are the declared types, and registers the variables it always did."""
import glob
import hashlib
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = sorted(os.path.relpath(p, ROOT) for pat in ("configs/*.config", "configs/vgg16/*.config")
                 for p in glob.glob(os.path.join(ROOT, pat)))
# feature_extractor.type -> (the extractor's out_act, its towers' out_act)
OUT_ACT = {"faster_rcnn_resnet50": ("relu", "relu"), "faster_rcnn_resnet101": ("relu", "relu"),
           "faster_rcnn_inception_resnet_v2": ("relu", "relu"), "frcnn_mobilenet_v1": ("relu6", "relu6"),
           "faster_rcnn_vgg_16": ("relu", None)}


def specs_digest(specs):
    """(count, sha256) over name, shape, trainable and weight decay of every VarSpec, in registration order."""
    text = "".join("%s %s %d %r\n" % (s.name, "x".join(map(str, s.shape)), s.trainable, s.weight_decay) for s in specs)
    return {"count": len(specs), "sha256": hashlib.sha256(text.encode()).hexdigest()}


def test_every_config_is_covered():
    assert len(CONFIGS) == 10
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "variable_specs_digest.json")))
    assert sorted(golden) == sorted("%s:%s" % (c, m) for c in CONFIGS for m in ("train", "inference"))


@pytest.mark.parametrize("is_training", [True, False], ids=["train", "inference"])
@pytest.mark.parametrize("cfg_path", CONFIGS)
def test_model_parts_are_the_declared_types(cfg_path, is_training):
    from mtl_ssl_amd import config, model_builder, nn
    cfg = config.parse_pipeline_config(open(os.path.join(ROOT, cfg_path)).read())
    model, ps = model_builder._construct(cfg.model, is_training, 0)
    assert model.layers and all(isinstance(l, nn.Layer) for l in model.layers)
    fe_act, tower_act = OUT_ACT[cfg.model.faster_rcnn.feature_extractor.type]
    towers = [t for t in (model.tower, model.closeness_tower, model.window_tower) if t is not None]
    assert towers
    for t in towers:
        assert isinstance(t, nn.Tower) and t.out_act == tower_act
    fe = model._feature_extractor
    assert isinstance(fe, nn.FeatureExtractor) and fe.out_act == fe_act
    # the same variables — names, shapes, order (and trainable flag, weight decay) — as before the types existed
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "variable_specs_digest.json")))
    assert specs_digest(ps.specs) == golden["%s:%s" % (cfg_path, "train" if is_training else "inference")]
    assert specs_digest(model_builder.variable_specs(cfg.model, is_training)) == specs_digest(ps.specs)
