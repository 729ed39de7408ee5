"""Faster R-CNN VGG-16 feature extractor over the HIP conv family.

Restates object_detection/models/faster_rcnn_vgg_16_feature_extractor.py:36-140 and slim/nets/vgg.py:52-216
(`vgg_16_base(final_endpoint='conv5')`): five groups of 3x3 / 1 SAME convolutions with biases and ReLU (2, 2, 3, 3, 3
layers of 64, 128, 256, 512, 512 channels), a 2x2 / 2 VALID max-pool after groups 1-4, `conv5_3` (512 channels at
stride 16) for the RPN. The second-stage "tower" is tf.identity: the pooled RoI crops go straight to the predictor.

What the reference's builder cannot do (it passes a `batch_norm_trainable` the constructor does not take, and the
proto's `freeze_layer` default 'block1' dies in int('k1')) is decided in DESIGN.md §7.
"""
import torch

from . import nn, ops

# slim/nets/vgg.py:141-153: (convolutions, channels) per group
_GROUPS = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))
_INIT = ("variance_scaling", 1.0, "FAN_AVG", True)          # slim.conv2d's default: xavier_initializer (uniform)
FREEZE_LAYERS = ("",) + tuple("conv%d" % g for g in range(1, len(_GROUPS) + 1))


def trainable_groups(freeze_layer, is_training):
    """utils/kwargs_util.py:6-18: '' trains every group, 'convN' trains group g iff g > N; nothing trains outside
    training. Any other value (the proto default 'block1' included) is refused."""
    if freeze_layer not in FREEZE_LAYERS:
        raise ValueError("faster_rcnn_vgg_16: feature_extractor.freeze_layer must be one of %s, got %r — the proto default "
                         "'block1' names a ResNet block, so a VGG config must set the field"
                         % (", ".join(repr(v) for v in FREEZE_LAYERS), freeze_layer))
    n = int(freeze_layer[-1]) if freeze_layer else 0
    return [bool(is_training) and g > n for g in range(1, len(_GROUPS) + 1)]


class IdentityTower(nn.Tower):
    """models/faster_rcnn_vgg_16_feature_extractor.py:76-81: `_extract_box_classifier_features` is tf.identity. No
    variables; the output is NOT an activation of the tower's own (`out_act` None): it is a bilinear crop of a ReLU map,
    full of exact zeros through which the predictor's gradient must pass."""
    out_act = None
    trainable = False

    def __init__(self, cin):
        self.cout = cin

    def layers(self):
        return []

    def forward(self, crops, save):
        return crops, None

    def backward(self, g_out, out, ctx, need_input_grad, masked=False, wgrad=nn.INLINE_WGRAD, active=None):
        return g_out if need_input_grad else None


class FasterRCNNVgg16FeatureExtractor(nn.FeatureExtractor):
    channel_means = (102.9801, 115.9465, 122.7717)         # Caffe's, per BGR channel (:43-49)
    out_act = "relu"
    supports_rfcn = False          # RFCNMetaArch refuses an extractor whose second-stage tower is the identity

    def __init__(self, ps, is_training, first_stage_features_stride=16, weight_decay=0.0005, freeze_layer="",
                 first_stage_scope="FirstStageFeatureExtractor"):
        # the stride is checked and otherwise unused (:86-108): the trunk is always conv5_3 at stride 16
        super().__init__(ps, bool(is_training), first_stage_features_stride, weight_decay)
        self.group_trainable = trainable_groups(freeze_layer, is_training)
        self.groups = []
        cin = 3
        for g, (n, cout) in enumerate(_GROUPS, 1):
            convs = []
            for i in range(1, n + 1):
                convs.append(nn.Conv(ps, "%s/vgg_16/conv%d/conv%d_%d" % (first_stage_scope, g, g, i), cin, cout, 3, _INIT,
                                     self.group_trainable[g - 1], weight_decay, activation="relu"))
                cin = cout
            self.groups.append(convs)
        self.cout = cin
        # the backward pass stops below the first trainable group (a later group of a 'convN' freeze always trains)
        self.first_trainable = next((g for g, t in enumerate(self.group_trainable) if t), len(_GROUPS))
        self._means = None

    def layers(self):
        return [l for convs in self.groups for l in convs]

    def preprocess(self, resized_inputs):
        """RGB -> BGR, then Caffe's per-channel means (:43-49), one launch."""
        if self._means is None:
            self._means = torch.tensor(self.channel_means, dtype=torch.float32, device=resized_inputs.device)
        return ops.preprocess_bgr(resized_inputs.contiguous(), self._means)

    def extract_proposal_features(self, x, save=True):
        """-> (conv5_3 after its ReLU, ctx). ctx, kept only for the trainable groups: per group (the inputs of its
        convolutions, its last activation, the pooled map, the pool's pads)."""
        self.check_inputs(x)
        ctx = []
        for g, convs in enumerate(self.groups):
            keep = save and self.is_training and g >= self.first_trainable
            xs = []
            for l in convs:
                xs.append(x)
                x = l.forward(x)
            last, pooled, pads = x, None, None
            if g < len(self.groups) - 1:
                pooled, pads = ops.maxpool_fwd(x, 2, 2, "VALID")
                x = pooled
            ctx.append((xs, last, pooled, pads) if keep else None)
        return x, (ctx if save else None)

    def backward_proposal_features(self, gp, ctx, wgrad=nn.INLINE_WGRAD):
        """gp: dL/d(pre-activation of conv5_3) (already ReLU-masked). Inside a group the dgrad epilogue masks by the
        input activation. Across a pool the next group's first dgrad is masked by the POOLED map — it is positive exactly
        where the element that receives the gradient is — and the plain max-pool backward routes it. The filter gradients
        run inline, whatever `wgrad` is."""
        if not self.is_training:
            return
        for g in range(len(self.groups) - 1, self.first_trainable - 1, -1):
            xs, last, pooled, pads = ctx[g]
            if pooled is not None:
                gp = ops.maxpool_bwd(last, pooled, gp, 2, 2, pads)
            convs = self.groups[g]
            for i in range(len(convs) - 1, -1, -1):
                convs[i].wgrad(xs[i], gp)
                if i == 0 and g == self.first_trainable:
                    return                      # nothing below trains, and the image never gets a gradient
                gp = convs[i].dgrad(xs[i].shape, gp, mask_ref=xs[i])

    def box_classifier_tower(self, scope, trainable):
        return IdentityTower(self.cout)
