"""The VGG-16 extractor restated for the whole-step oracle (test infrastructure; a plain module, no fixtures).

`VggOracle` is oracle.model.Oracle with the trunk and the second-stage tower of
object_detection/models/faster_rcnn_vgg_16_feature_extractor.py + slim/nets/vgg.py:52-216: BGR preprocessing with
Caffe's means, five groups of 3x3 SAME convolutions with biases and ReLU, a 2x2 / 2 VALID max-pool after groups 1-4, and
an identity tower. parity_report.oracle_on_device_rpn / against_float64 take it as they take Oracle."""
import os

import numpy as np
import torch

from oracle import ops_torch as T
from oracle.model import MEANS, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SMOKE = os.path.join(ROOT, "configs", "vgg16", "smoke_vgg16_mtl.config")
GROUPS = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))
BGR_MEANS = (102.9801, 115.9465, 122.7717)
SCOPE = "FirstStageFeatureExtractor/vgg_16"


def trunk_names():
    """The 26 trunk variables in registration order with their shapes."""
    out, cin = [], 3
    for g, (n, cout) in enumerate(GROUPS, 1):
        for i in range(1, n + 1):
            s = "%s/conv%d/conv%d_%d" % (SCOPE, g, g, i)
            out += [(s + "/weights", (3, 3, cin, cout)), (s + "/biases", (cout,))]
            cin = cout
    return out


class VggOracle(Oracle):
    def __init__(self, hp, values, dtype=np.float32):
        super().__init__(hp, values, dtype)
        self.tower_inputs = []            # (scope, crops) of every tower call, crops with their gradient retained

    def preprocess(self, rgb):
        """models/faster_rcnn_vgg_16_feature_extractor.py:43-49: RGB -> BGR, minus Caffe's means."""
        return torch.flip(rgb, dims=[3]) - torch.tensor(np.asarray(BGR_MEANS, np.float32)).to(rgb.dtype)

    def trunk_from_rgb(self, rgb):
        x = self.preprocess(rgb)
        for g, (n, _) in enumerate(GROUPS, 1):
            for i in range(1, n + 1):
                s = "%s/conv%d/conv%d_%d" % (SCOPE, g, g, i)
                x = torch.relu(T.conv2d(x, self.v[s + "/weights"], 1, 1, "SAME") + self.v[s + "/biases"])
            if g < len(GROUPS):
                x = T.max_pool(x, 2, 2, "VALID")
        return x

    def trunk(self, x):
        """Oracle.step / detect hand over img - MEANS (the ResNet extractor's preprocessing): undone first."""
        return self.trunk_from_rgb(x + torch.tensor(MEANS).to(x.dtype))

    def tower(self, crops, scope):
        """tf.identity (:76-81). x + 0 is x in a node of its own: its retained gradient is what THIS head sends back
        (the main and the closeness head read the same crops)."""
        out = crops + 0
        if out.requires_grad:
            out.retain_grad()
        self.tower_inputs.append((scope, out))
        return out


TRUNK_SEED = 7          # see trunk_case


def trunk_case(hw, seed=TRUNK_SEED):
    """Inputs of the stand-alone trunk tests: B = 2 images of size `hw` with values in [0, 255], the 26 variables from
    the extractor's own initialisers, and an upstream gradient for conv5_3's output.
    TRUNK_SEED was checked on the CPU for both image sizes of tests/vgg/test_gpu_detection.py: the torch-CPU fp32 run of
    VggOracle has no variable beyond 1e-3 relative L2 of the float64 run (worst 2e-6), so a variable beyond it on the
    device is the device's doing, not an activation flip that any fp32 evaluation of this case shows."""
    from mtl_ssl_amd import params
    rng = np.random.RandomState(seed * 1000 + hw[0])
    imgs = rng.uniform(0.0, 255.0, (2, hw[0], hw[1], 3)).astype(np.float32)
    values = {n: params.init_value(params.VarSpec(n, s, ("variance_scaling", 1.0, "FAN_AVG", True)
                                                  if n.endswith("weights") else ("zeros",), True), seed)
              for n, s in trunk_names()}
    fh, fw = hw[0] // 16, hw[1] // 16
    g = rng.standard_normal((2, fh, fw, 512)).astype(np.float32)
    return imgs, values, g


def trunk_reference(imgs, values, g, dtype):
    """(feature map, {variable: gradient}) of sum(F * g) by autograd in `dtype`."""
    o = VggOracle({"arch": "vgg_16"}, values, dtype)
    F = o.trunk_from_rgb(torch.as_tensor(np.asarray(imgs, o.dtype)))
    (F * torch.as_tensor(np.asarray(g, o.dtype))).sum().backward()
    return F.detach().numpy(), {k: t.grad.numpy() for k, t in o.v.items() if t.grad is not None}


def hyper_params(cfg):
    """bench.hyper_params_for_oracle for a VGG config: that table knows the extractors it was written for, so it is asked
    about the same config under a ResNet name and the two entries that depend on the extractor are set here."""
    import bench
    fe = cfg.model.faster_rcnn.feature_extractor
    kept = fe["type"]
    fe["type"] = "faster_rcnn_resnet50"
    try:
        hp = bench.hyper_params_for_oracle(cfg)
    finally:
        fe["type"] = kept
    hp["arch"] = "vgg_16"
    fr, mtl = cfg.model.faster_rcnn, cfg.model.mtl
    for scope, bp in (("SecondStageBoxPredictor", fr.second_stage_box_predictor),
                      ("ClosenessBoxPredictor", mtl.closeness_box_predictor),
                      ("WindowBoxPredictor", mtl.window_box_predictor)):
        spec = hp["predictors"][scope]
        if spec:
            m = bp.mask_rcnn_box_predictor
            spec["depth"] = max(min(512, int(m.max_depth)), int(m.min_depth))       # the identity tower's 512 channels
            spec["n_extra"] = int(m.num_layers_before_predictor) if spec["depth"] > 0 else 0
    return hp


def smoke_config(extra_mtl=""):
    """The parsed smoke configuration; `extra_mtl` is text appended inside `mtl { }` (later fields win)."""
    from mtl_ssl_amd import config
    text = open(SMOKE).read()
    if extra_mtl:
        text = text.replace("stop_gradient_for_aux_tasks: false", extra_mtl, 1)
        assert extra_mtl in text
    return config.parse_pipeline_config(text)
