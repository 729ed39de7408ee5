"""Layer objects with explicit forward/backward over the C-ABI kernels (no autograd, no tracing).

Gradient convention between residual units: `backward(gp)` receives gp = dL/d(pre-activation of
the unit's output) — i.e. already multiplied by the ReLU mask of the unit's output — and returns
the same quantity for the unit's input. The ReLU masks are applied in the dgrad epilogues, so
there are no stand-alone elementwise backward kernels in the trunk.

Frozen BatchNorm (the reference always runs BN in inference mode during detector training,
models/faster_rcnn_resnet_v1_feature_extractor.py:138,171) is folded: w_eff = w * scale[k],
y = conv(x, w_eff) + shift[k]; dW = scale[k] * wgrad(x, g).

The one normaliser that runs on batch statistics is the heads' (BatchNorm below: a hyperparams block's `batch_norm`):
bias-free conv, then ops.batch_norm_train_fwd; its backward applies the activation's mask itself.
"""
import torch

from . import ops

f32 = torch.float32


def _refresh_bn(layer):
    """Recompute scale/shift in place after an optimizer step moved gamma/beta."""
    if layer.bn_trainable:
        ps = layer.ps
        if layer.gamma is not None:
            torch.mul(ps.value(layer.gamma.name), layer.inv_std, out=layer.scale)
        torch.addcmul(ps.value(layer.beta.name), ps.value(layer.mean.name), layer.scale, value=-1.0,
                      out=layer.shift)


class WgradStream:
    """Filter gradients off the critical path: `run(layer, x, g)` enqueues layer.wgrad(x, g) on a side HIP
    stream behind an event on the issuing stream. The backward chain of the B=2 trunk is a string of small
    GEMMs (4 864 pixels) in which each dgrad waits for the previous one while the wgrads feed nothing but the
    optimizer; taken out of that chain they fill the CUs the chain leaves idle. The caller joins the stream
    before the optimizer (FasterRCNNMetaArch.backward) and lists it in compute_streams() for the reducer."""

    def __init__(self, stream):
        self.stream = stream

    def run(self, layer, x, g, **kw):
        if not layer.trainable:
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.stream.wait_event(ev)
        for t in (x, g) + tuple(kw.values()):  # keep the caching allocator from recycling them under the side stream
            t.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            layer.wgrad(x, g, **kw)


class _InlineWgrad:
    stream = None

    @staticmethod
    def run(layer, x, g, **kw):
        layer.wgrad(x, g, **kw)


INLINE_WGRAD = _InlineWgrad()


_ACT_EPILOGUE = {None: 0, "relu": ops.EPI_RELU, "relu6": ops.EPI_RELU6, "tanh": ops.EPI_TANH}


def act_epilogue(act):
    """The forward epilogue flag of an output activation: 'relu' | 'relu6' | 'tanh' | None."""
    return _ACT_EPILOGUE[act]


def dgrad_epilogue(residual=None, accum=False, mask_ref=None, mask6=False):
    """The epilogue flags of an input gradient: + residual, accumulate into `out`, masked by (mask_ref > 0), or by
    (0 < mask_ref < 6) with mask6."""
    return ((ops.EPI_RESIDUAL if residual is not None else 0) | (ops.EPI_ACCUM if accum else 0)
            | ((ops.EPI_MASK6 if mask6 else ops.EPI_MASK) if mask_ref is not None else 0))


class Layer:
    """What every element of `model.layers` is. A subclass registers its variables in __init__ (host
    only), allocates in prepare(), and supplies geometry() for the one cached desc()."""
    trainable = False            # the filter `w` (and the bias that goes with it) receives a gradient
    bn_trainable = False         # gamma / beta receive gradients (the moving statistics never do)
    gamma = beta = None
    w_eff = None                 # the filter the kernels read when it is a folded shadow copy of `w`
    # > 0: this layer's output is a channel slice of a concatenated map with `ldy` channels (set by the owner of the
    # concat before the first call): forward(out=view) writes it in place, dgrad / wgrad read dy views in place
    ldy = 0

    def __init__(self):
        self._desc = {}

    def prepare(self):
        """Allocate what depends on the finalized ParamStore (shadow filters, normaliser constants)."""

    def refold(self):
        """Recompute the normaliser constants after an optimizer step (the CPU path of FasterRCNNMetaArch.refold)."""

    def wgrad(self, x, g):
        """Accumulate the gradients of the layer's variables and report them final (ParamStore.grad_ready)."""

    def grad_vars(self):
        """The variables of this layer that receive a gradient: the filter if it trains (a bias trains, and is reported,
        with its filter), gamma / beta if the normaliser's parameters train."""
        bn = (self.gamma, self.beta) if self.bn_trainable else ()
        return tuple(v for v in ((self.w,) if self.trainable else ()) + bn if v is not None)

    def geometry(self):
        """-> (filter shape [kh, kw, C, K], stride, dilation, padding) of the layer's convolution."""
        raise NotImplementedError

    def desc(self, shape):
        d = self._desc.get(tuple(shape))
        if d is None:
            d = self._desc[tuple(shape)] = ops.conv_desc(shape, *self.geometry(), ldy=self.ldy)
        return d


class _FrozenBN(Layer):
    """A filter followed by slim.batch_norm in inference mode, folded (module docstring): the normaliser's variables and
    constants, stated once for ConvBN and DepthwiseBN."""

    def _add_batch_norm(self, c, gamma_init, bn_scale=True):
        ps, bn, t = self.ps, self.scope + "/BatchNorm/", self.bn_trainable
        if bn_scale:
            self.gamma = ps.add(bn + "gamma", (c,), ("uniform", 0.8 * gamma_init, 1.2 * gamma_init), t)
        self.beta = ps.add(bn + "beta", (c,), ("uniform", -0.1, 0.1), t)
        self.mean = ps.add(bn + "moving_mean", (c,), ("uniform", -0.1, 0.1), False)
        self.var = ps.add(bn + "moving_variance", (c,), ("uniform", 0.8, 1.2), False)

    def prepare(self):
        """w_eff in the shape the layer's kernels read: `w_eff_shape`."""
        ps = self.ps
        b = ps.value(self.beta.name) if self.beta is not None else 0.0      # no beta: slim.batch_norm(center=False)
        m, v = ps.value(self.mean.name), ps.value(self.var.name)
        self.inv_std = torch.rsqrt(v + self.eps)
        self.scale = ((ps.value(self.gamma.name) * self.inv_std) if self.gamma is not None
                      else self.inv_std.clone()).contiguous()
        self.shift = (b - m * self.scale).contiguous()
        if self.w.trainable:       # refreshed by the batched fold (ops.fold_scales) after each update
            self.w_eff = ps.register_fold(self.w, self.scale).view(self.w_eff_shape)
        else:
            self.w_eff = torch.empty(self.w_eff_shape, dtype=f32, device=ps.device)
            ops.scale_channels(ps.value(self.w.name).view(self.w_eff_shape), self.scale, self.w_eff)

    def refold(self):
        _refresh_bn(self)

    def bn_grad(self, y, gp):
        """d(gamma), d(beta) of the inference-mode normaliser from the layer output `y` and
        gp = dL/d(pre-activation) (slim arg-scopes that leave BatchNorm trainable: MobileNet)."""
        if self.bn_trainable and self.gamma is not None:
            ps = self.ps
            ops.bn_param_grads(y, gp, ps.value(self.gamma.name), ps.value(self.beta.name),
                               ps.grad(self.gamma.name), ps.grad(self.beta.name), beta=1.0)
            ps.grad_ready(self.gamma, self.beta)


class ConvBN(_FrozenBN):
    """slim.conv2d + frozen slim.batch_norm (+ReLU) — slim/nets/resnet_v1.py:102-119."""

    def __init__(self, ps, scope, cin, cout, k, stride=1, dilation=1, padding="SAME",
                 trainable=True, weight_decay=0.0, eps=1e-5, gamma_init=1.0, relu=True, act=None,
                 init=("variance_scaling", 2.0, "FAN_IN", False), bn_trainable=False,
                 weights_name="weights", bn_scale=True):
        """k: int or (kh, kw). bn_scale=False: slim.batch_norm(scale=False) — no gamma variable
        (Inception arg scopes); bn_trainable: gamma/beta receive gradients (moving stats never do)."""
        super().__init__()
        self.ps, self.scope = ps, scope
        self.bn_trainable = bn_trainable
        self.k, self.stride, self.dilation, self.padding, self.eps = k, stride, dilation, padding, eps
        self.trainable = trainable
        self.act = act if act is not None else ("relu" if relu else None)     # 'relu' | 'relu6' | None
        self.relu = self.act is not None
        kh, kw = k if isinstance(k, tuple) else (k, k)
        self.w = ps.add(scope + "/" + weights_name, (kh, kw, cin, cout), init, trainable, weight_decay)
        self.w_eff_shape = self.w.shape
        self._add_batch_norm(cout, gamma_init, bn_scale)
        self._kept = {}          # x.data_ptr() -> (Winograd-transformed x, variant), between forward(keep=True) and wgrad

    def geometry(self):
        return self.w.shape, self.stride, self.dilation, self.padding

    def forward(self, x, residual=None, relu=None, keep=False, out=None):
        """keep: this forward will be followed by wgrad(x, .) of the same x (training with saved activations) —
        a Winograd layer then keeps its transformed input for the filter gradient.
        out: where to write (required when self.ldy is set: the layer's slice of the concatenated map)."""
        act = self.act if relu is None else ("relu" if relu else None)
        epi = ops.EPI_BIAS | act_epilogue(act) | (ops.EPI_RESIDUAL if residual is not None else 0)
        return ops.conv2d_fwd(self.desc(x.shape), x, self.w_eff, self.shift, residual, epi, out=out,
                              xf_cache=self.ps.filter_cache,
                              keep_input_xf=self._keep_slot() if (keep and self.trainable and self.k == 3) else None)

    def _keep_slot(self):
        if len(self._kept) > 8:      # forwards whose backward never came (a caller that saves and then drops the step)
            self._kept.clear()
        return self._kept

    def wgrad(self, x, g, active=None):
        """active: uint8 flag per image (RoI) of g, 0 = its rows of g are all exactly zero (ops.conv2d_wgrad), or None."""
        if self.trainable:
            # without a gamma, d(beta) is just the column sum of g: ride on the wgrad's dbias pass
            db = self.ps.grad(self.beta.name) if (self.bn_trainable and self.gamma is None) else None
            ops.conv2d_wgrad(self.desc(x.shape), x, g, self.ps.grad(self.w.name), out_scale=self.scale,
                             dbias=db, beta=1.0, input_xf=self._kept.pop(x.data_ptr(), None), active=active)
            self.ps.grad_ready(self.w, self.beta if db is not None else None)

    def dgrad(self, x_shape, g, residual=None, mask_ref=None, out=None, accum=False, mask6=False, active=None):
        return ops.conv2d_dgrad(self.desc(x_shape), g, self.w_eff, residual, mask_ref,
                                dgrad_epilogue(residual, accum, mask_ref, mask6), out=out, xf_cache=self.ps.filter_cache,
                                active=active)


class DepthwiseBN(_FrozenBN):
    """slim.separable_conv2d(num_outputs=None, depth_multiplier=1) + frozen batch_norm + ReLU6
    (slim/nets/mobilenet_v1.py:229-245). Filter [k,k,C,1] named `depthwise_weights` like slim."""

    def __init__(self, ps, scope, c, k=3, stride=1, dilation=1, trainable=True, weight_decay=0.0, eps=1e-3,
                 act="relu6", init=("truncated_normal", 0.09), bn_trainable=False, gamma_init=1.0, batch_norm=True):
        """batch_norm=False: the bare filter — no normaliser variables; the subclass supplies prepare / forward."""
        super().__init__()
        self.ps, self.scope, self.c = ps, scope, c
        self.bn_trainable = bn_trainable
        self.k, self.stride, self.dilation, self.eps, self.act = k, stride, dilation, eps, act
        self.trainable = trainable
        self.w = ps.add(scope + "/depthwise_weights", (k, k, c, 1), init, trainable, weight_decay)
        self.w_eff_shape = (k, k, c)
        if batch_norm:
            self._add_batch_norm(c, gamma_init)

    def geometry(self):
        return (self.k, self.k, self.c, self.c), self.stride, self.dilation, "SAME"

    def forward(self, x):
        return ops.depthwise_fwd(self.desc(x.shape), x, self.w_eff, self.shift, ops.EPI_BIAS | act_epilogue(self.act))

    def wgrad(self, x, g):
        if self.trainable:
            ops.depthwise_wgrad(self.desc(x.shape), x, g, self.ps.grad(self.w.name), out_scale=self.scale,
                                beta=1.0)
            self.ps.grad_ready(self.w)

    def dgrad(self, x_shape, g, mask_ref=None, mask6=False):
        return ops.depthwise_dgrad(self.desc(x_shape), g, self.w_eff, mask_ref,
                                   dgrad_epilogue(None, False, mask_ref, mask6))


class BatchNorm(_FrozenBN):
    """slim.batch_norm as the normalizer_fn of a hyperparams block that has `batch_norm { decay center scale epsilon
    train }` (protos/hyperparams.proto:101-110, builders/hyperparams_builder.py:56-76, 156-175): the normaliser of ONE
    filter without bias (nn.Conv(batch_norm=...)), which owns <layer scope>/BatchNorm/{beta, gamma, moving_mean,
    moving_variance} — beta only with `center`, gamma only with `scale`; slim's initial values 0, 1, 0, 1. Two modes:

    * batch statistics (`batch_stats`: is_training and batch_norm.train): y = act(gamma * xhat + beta) over the rows of
      the per-GPU batch (ops.batch_norm_train_fwd / _bwd; nothing is synchronised between ranks), and — only where the
      caller asks (`update`: the training step's forward) — the moving averages move by
      assign_moving_average(zero_debias=False). Training never reads the moving values;
    * frozen (is_training False — eval, export, Detector — or train: false): the moving statistics, folded into the
      filter exactly as _FrozenBN does for the trunks (prepare / refold are its own).

    gamma / beta are trainable iff is_training, whatever `train` says ('trainable': is_training, builder line 173) and
    whether or not the filter is. DESIGN.md §7 (parity with TF 1.7 is unpinned)."""

    def __init__(self, cfg, is_training):
        super().__init__()
        self.decay, self.eps = float(cfg.decay), float(cfg.epsilon)
        self.center, self.with_scale = bool(cfg.center), bool(cfg.scale)
        self.batch_stats = bool(is_training and cfg.train)
        self.bn_trainable = bool(is_training)
        self.f = ops.moving_average_factor(self.decay)

    def bind(self, layer, field="batch_norm"):
        """Registers the variables behind the filter of `layer` (an nn.Conv), in slim's order."""
        if layer.activation not in (None, "relu", "relu6"):
            raise ValueError("%s: batch_norm is built with RELU, RELU_6 or NONE activations" % field)
        ps, c = layer.ps, layer.cout
        self.ps, self.scope, self.w, self.trainable = ps, layer.scope, layer.w, layer.trainable
        self.w_eff_shape = (1, 1, layer.cin, c) if layer.fc else layer.w.shape
        if self.bn_trainable and not self.batch_stats and (not self.center or c % 4 != 0):
            # the gradients of a folded normaliser's gamma / beta come from ops.bn_param_grads (channel quads, y - beta)
            raise ValueError("%s: train: false while training is built for center: true and a layer width that is a "
                             "multiple of 4 (%s has %d)" % (field, layer.scope, c))
        bn, t = layer.scope + "/BatchNorm/", self.bn_trainable
        if self.center:
            self.beta = ps.add(bn + "beta", (c,), ("zeros",), t)
        if self.with_scale:
            self.gamma = ps.add(bn + "gamma", (c,), ("const", 1.0), t)
        self.mean = ps.add(bn + "moving_mean", (c,), ("zeros",), False)
        self.var = ps.add(bn + "moving_variance", (c,), ("const", 1.0), False)
        return self

    def param_vars(self):
        return tuple(v for v in (self.gamma, self.beta) if v is not None and self.bn_trainable)

    def prepare(self):
        if not self.batch_stats:
            super().prepare()

    def refold(self):
        if not self.batch_stats:
            super().refold()

    def _values(self, *specs):
        return tuple(None if s is None else self.ps.value(s.name) for s in specs)

    def forward(self, z, act, update, keep):
        """Batch-statistics mode. z: the filter's bias-free output [..., C]. keep: a dict that receives what backward
        reads, or None. update: move the moving averages (the training step's forward only)."""
        gamma, beta = self._values(self.gamma, self.beta)
        mm, mv = self._values(self.mean, self.var) if update else (None, None)
        y, mean, inv_std = ops.batch_norm_train_fwd(z, gamma, beta, self.eps, act_epilogue(act), mm, mv, self.f)
        if keep is not None:
            keep.update(z=z, mean=mean, inv_std=inv_std)
        return y

    def backward(self, keep, y, g, act):
        """Batch-statistics mode. g = dL/dy (the activation's mask is applied inside, from y) -> dL/dz; accumulates and
        reports the gradients of gamma / beta."""
        ps = self.ps
        mask = {None: 0, "relu": ops.EPI_MASK, "relu6": ops.EPI_MASK6}[act]
        dg, db = (None if s is None else ps.grad(s.name) for s in (self.gamma, self.beta))
        dz = ops.batch_norm_train_bwd(keep["z"], g.view(keep["z"].shape), self._values(self.gamma)[0], keep["mean"],
                                      keep["inv_std"], dg, db, y=y.view(keep["z"].shape) if mask else None,
                                      mask_epilogue=mask, accum=1.0)
        ps.grad_ready(self.gamma, self.beta)
        return dz.view(g.shape)

    def frozen_param_grads(self, y, gp):
        """Frozen mode while training (train: false): gamma / beta gradients of the folded normaliser from the layer's
        output y and gp = dL/d(pre-activation)."""
        if self.batch_stats or not self.bn_trainable:
            return
        ps, c = self.ps, y.shape[-1]
        db = ps.grad(self.beta.name)
        if self.gamma is not None:
            gamma, dg = ps.value(self.gamma.name), ps.grad(self.gamma.name)
        else:
            gamma, dg = torch.ones_like(db), torch.zeros_like(db)
        ops.bn_param_grads(y.view(-1, c), gp.view(-1, c), gamma, ps.value(self.beta.name), dg, db, beta=1.0)
        ps.grad_ready(self.gamma, self.beta)


def _of_folded_norm(name):
    """A Layer attribute of the folded normaliser, read from the layer's `norm` while that runs on the moving
    statistics (the batched refresh and fold of the model read them off the layer); the Layer default otherwise."""
    def get(self):
        n = self.norm
        return getattr(n, name) if (n is not None and not n.batch_stats) else getattr(Layer, name, None)
    return property(get)


class Conv(Layer):
    """slim.conv2d / slim.fully_connected of the heads (RPN conv, predictors, refiner): with biases and no normaliser, or
    — batch_norm given: the nn.BatchNorm of a hyperparams block — the filter without bias followed by that normaliser
    and the activation. A layer without one runs exactly the code it ran before normalisers existed."""
    gamma, beta, mean, inv_std, scale, shift, w_eff, bn_trainable = (
        _of_folded_norm(k) for k in ("gamma", "beta", "mean", "inv_std", "scale", "shift", "w_eff", "bn_trainable"))

    def __init__(self, ps, scope, cin, cout, k, init, trainable=True, weight_decay=0.0,
                 activation=None, fc=False, rate=1, batch_norm=None):
        super().__init__()
        self.ps, self.scope, self.k, self.trainable, self.activation = ps, scope, k, trainable, activation
        self.rate = rate
        shape = (cin, cout) if fc else (k, k, cin, cout)
        self.fc = fc
        self.w = ps.add(scope + "/weights", shape, init, trainable, weight_decay)
        self.cin, self.cout = cin, cout
        self.b = self.norm = None
        if batch_norm is None:
            self.b = ps.add(scope + "/biases", (cout,), ("zeros",), trainable)
        else:
            self.norm = batch_norm.bind(self)

    @property
    def batch_stats(self):
        """The layer normalises with batch statistics: forward takes `keep` / `update`, and norm_backward applies the
        activation's mask itself (the caller passes dL/d(output), unmasked)."""
        return self.norm is not None and self.norm.batch_stats

    def grad_vars(self):
        return super().grad_vars() + (self.norm.param_vars() if self.batch_stats else ())

    def prepare(self):
        if self.norm is not None:
            self.norm.prepare()

    def refold(self):
        if self.norm is not None:
            self.norm.refold()

    def _w4(self):
        w = self.ps.value(self.w.name)
        return w.view(1, 1, self.cin, self.cout) if self.fc else w

    def geometry(self):
        return (self.k, self.k, self.cin, self.cout), 1, self.rate, "SAME"

    def forward(self, x, keep=None, update=False):
        """x: NHWC, or [rows, cin] for fc=True (treated as rows x 1 x 1 x cin). keep / update: BatchNorm.forward's, for
        a layer that normalises with batch statistics."""
        x4 = x.view(x.shape[0], 1, 1, self.cin) if self.fc else x
        n, act = self.norm, act_epilogue(self.activation)
        if n is None:
            y = ops.conv2d_fwd(self.desc(x4.shape), x4, self._w4(), self.ps.value(self.b.name), None,
                               ops.EPI_BIAS | act, xf_cache=self.ps.filter_cache)
        elif n.batch_stats:
            z = ops.conv2d_fwd(self.desc(x4.shape), x4, self._w4(), None, None, 0, xf_cache=self.ps.filter_cache)
            y = n.forward(z, self.activation, update, keep)
        else:
            y = ops.conv2d_fwd(self.desc(x4.shape), x4, n.w_eff, n.shift, None, ops.EPI_BIAS | act,
                               xf_cache=self.ps.filter_cache)
        return y.view(x.shape[0], self.cout) if self.fc else y

    def norm_backward(self, keep, y, g):
        """The normaliser's backward, before wgrad / dgrad, for a layer that has one -> dL/d(filter output).
        Batch statistics: g = dL/dy, the activation's mask is applied inside. Frozen: g = dL/d(pre-activation), masked by
        the caller as for a layer without normaliser, and comes back unchanged. Either way gamma / beta get their
        gradients."""
        if self.norm.batch_stats:
            return self.norm.backward(keep, y, g, self.activation)
        self.norm.frozen_param_grads(y, g)
        return g

    def wgrad(self, x, g):
        if not self.trainable:
            return
        x4 = x.view(x.shape[0], 1, 1, self.cin) if self.fc else x
        g4 = g.view(g.shape[0], 1, 1, self.cout) if self.fc else g
        gw = self.ps.grad(self.w.name).view(self.k, self.k, self.cin, self.cout)
        if self.norm is None:
            ops.conv2d_wgrad(self.desc(x4.shape), x4, g4, gw, dbias=self.ps.grad(self.b.name), beta=1.0)
        else:         # no bias; a folded normaliser's scale reaches the filter gradient
            ops.conv2d_wgrad(self.desc(x4.shape), x4, g4, gw, out_scale=self.scale, beta=1.0)
        self.ps.grad_ready(self.w, self.b)

    def dgrad(self, x_shape, g, residual=None, mask_ref=None, out=None, accum=False, mask6=False):
        x4s = (x_shape[0], 1, 1, self.cin) if self.fc else tuple(x_shape)
        g4 = g.view(g.shape[0], 1, 1, self.cout) if self.fc else g
        w = self.w_eff if self.w_eff is not None else self._w4()
        dx = ops.conv2d_dgrad(self.desc(x4s), g4, w, residual, mask_ref,
                              dgrad_epilogue(residual, accum, mask_ref, mask6), out=out, xf_cache=self.ps.filter_cache)
        return dx.view(x_shape) if self.fc else dx


DROPOUT_SEED_SALT = 0x6D2B79F5


def dropout_stream(step, slot):
    """Counter-hash (seed salt, stream id) of a dropout layer. Dropout draws live in a hash domain of their own: the
    model seed is XOR-ed with DROPOUT_SEED_SALT (the samplers hash the plain seed with stream 2 * step * 65536 + k, which
    covers every 32-bit stream id over a long run — a bit partition of the stream id cannot keep the two apart); the
    stream id is 24 bits of step and 8 bits of layer slot. oracle/model.py restates the same formula."""
    return (((int(step) & 0xFFFFFF) << 8) | (int(slot) & 0xFF)) & 0xFFFFFFFF


class FCStack:
    """A run of slim.fully_connected(activation) layers, each optionally followed by slim.dropout — the refiner's
    `fc1..fcN` (faster_rcnn_meta_arch.py:835-839) and the predictors' `FC_i_depth` layers
    (core/box_predictor.py:479-488, 585-594). Explicit forward / backward over nn.Conv(fc=True)."""

    def __init__(self, ps, scopes, cin, widths, init, trainable, weight_decay, activation="relu", keep_prob=None,
                 slot0=0, batch_norm=None):
        """batch_norm: None, or a callable that makes the nn.BatchNorm of one layer (filter, normaliser, activation,
        dropout)."""
        if activation not in ("relu", None):
            raise ValueError("fully connected stacks support RELU or NONE activations, got %r" % (activation,))
        self.layers, self.activation = [], activation
        for scope, cout in zip(scopes, widths):
            self.layers.append(Conv(ps, scope, cin, cout, 1, init, trainable, weight_decay, activation=activation, fc=True,
                                    batch_norm=batch_norm() if batch_norm is not None else None))
            cin = cout
        self.cout = cin
        self.keep_prob = None if (keep_prob is None or keep_prob >= 1.0) else float(keep_prob)
        self.slot0 = slot0

    def forward(self, x, training, seed, step, update=False):
        """-> (output, ctx). Dropout acts only while training (slim.dropout's is_training). update: BatchNorm.forward's."""
        ctx = []
        for i, l in enumerate(self.layers):
            keep = {} if l.batch_stats else None
            a = l.forward(x, keep, update) if l.batch_stats else l.forward(x)
            drop = training and self.keep_prob is not None
            dseed = (int(seed) ^ DROPOUT_SEED_SALT) & 0xFFFFFFFF
            y = ops.dropout(a, self.keep_prob, dseed, dropout_stream(step, self.slot0 + i)) if drop else a
            ctx.append((x, a, (dseed, dropout_stream(step, self.slot0 + i)) if drop else None, keep))
            x = y
        return x, ctx

    def backward(self, ctx, g, need_input_grad=True):
        """g: dL/d(output). Accumulates the layers' filter / bias / normaliser gradients; returns dL/d(input) or None."""
        for i in range(len(self.layers) - 1, -1, -1):
            l = self.layers[i]
            x, a, drop, keep = ctx[i]
            if drop is not None:
                g = ops.dropout(g, self.keep_prob, drop[0], drop[1])
            if self.activation == "relu" and not l.batch_stats:
                g = ops.relu_bwd(a, g)
            if l.norm is not None:
                g = l.norm_backward(keep, a, g)
            l.wgrad(x, g)
            if i == 0 and not need_input_grad:
                return None
            g = l.dgrad(x.shape, g)
        return g


class Bottleneck:
    """slim/nets/resnet_v1.py:69-130 bottleneck (v1: BN after conv, stride in the 3x3)."""

    def __init__(self, ps, scope, cin, depth, depth_bottleneck, stride, rate=1, trainable=True,
                 weight_decay=0.0, bn_trainable=False):
        """bn_trainable: the unit's BatchNorm gamma / beta are trained (resnet_arg_scope(batch_norm_trainable=True),
        slim/nets/resnet_utils.py:203-237: a property of the normaliser, independent of `trainable`, which freezes
        the FILTERS of a block — a frozen block's gamma / beta still train); the statistics stay the moving ones."""
        s = scope + "/bottleneck_v1/"
        self.stride, self.cin, self.depth = stride, cin, depth
        self.shortcut = None
        if depth != cin:
            self.shortcut = ConvBN(ps, s + "shortcut", cin, depth, 1, stride, 1, "SAME", trainable,
                                   weight_decay, relu=False, bn_trainable=bn_trainable)
        self.conv1 = ConvBN(ps, s + "conv1", cin, depth_bottleneck, 1, 1, 1, "SAME", trainable, weight_decay,
                            bn_trainable=bn_trainable)
        self.conv2 = ConvBN(ps, s + "conv2", depth_bottleneck, depth_bottleneck, 3, stride, rate,
                            "RESNET_SAME", trainable, weight_decay, bn_trainable=bn_trainable)
        self.conv3 = ConvBN(ps, s + "conv3", depth_bottleneck, depth, 1, 1, 1, "SAME", trainable,
                            weight_decay, gamma_init=0.3, relu=True, bn_trainable=bn_trainable)
        self.trainable = trainable
        self.bn_trainable = bn_trainable

    def layers(self):
        return [l for l in (self.shortcut, self.conv1, self.conv2, self.conv3) if l is not None]

    def forward(self, x, save):
        if self.shortcut is not None:
            sc = self.shortcut.forward(x)
        elif self.stride > 1:
            sc, _ = ops.maxpool_fwd(x, 1, self.stride, "SAME")     # resnet_utils.subsample
        else:
            sc = x
        a1 = self.conv1.forward(x)
        a2 = self.conv2.forward(a1, keep=save)
        out = self.conv3.forward(a2, residual=sc)
        ctx = (x, a1, a2, sc if (self.shortcut is None and self.stride > 1) else None) if save else None
        if save and self.bn_trainable:
            # d(gamma) / d(beta) of conv3 and of the shortcut conv need the normalisers' own outputs: out - sc and sc
            ctx = ctx + (out, sc)
        return out, ctx

    def backward(self, gp, ctx, need_input_grad=True, mask_input=True, wgrad=INLINE_WGRAD, active=None):
        """gp: dL/d(pre-activation of out). Returns dL/d(pre-activation of x) (masked by x>0 when
        mask_input), or None. `wgrad`: where the filter gradients run (inline, or a WgradStream).
        active: uint8 flag per image (RoI), 0 = gp is exactly zero there — then so is every gradient of the unit, and the
        1x1 layers and a 3x3 layer on a Winograd plan leave those RoIs out (stride-1 units only: a RoI keeps its rows)."""
        kw = {} if active is None else dict(active=active)
        x, a1, a2, sc_sub = ctx[:4]
        if self.bn_trainable:
            out, sc = ctx[4], ctx[5]
            # conv3's normaliser output is out - sc wherever gp != 0 (gp is masked by out > 0, and there out is the
            # pre-activation sum); elsewhere the product with gp vanishes
            o3 = ops.axpby(sc, out.clone(), -1.0, 1.0)
            self.conv3.bn_grad(o3, gp)
            del o3
            if self.shortcut is not None:
                self.shortcut.bn_grad(sc, gp)
        wgrad.run(self.conv3, a2, gp, **kw)
        gp2 = self.conv3.dgrad(a2.shape, gp, mask_ref=a2, **kw)
        if self.bn_trainable:
            self.conv2.bn_grad(a2, gp2)
        wgrad.run(self.conv2, a1, gp2, **kw)
        gp1 = self.conv2.dgrad(a1.shape, gp2, mask_ref=a1, **kw)
        if self.bn_trainable:
            self.conv1.bn_grad(a1, gp1)
        wgrad.run(self.conv1, x, gp1, **kw)
        if self.shortcut is not None:
            wgrad.run(self.shortcut, x, gp, **kw)
        if not need_input_grad:
            return None
        if self.shortcut is not None:
            addend = self.shortcut.dgrad(x.shape, gp, **kw)
        elif self.stride > 1:
            addend = ops.maxpool_bwd(x, sc_sub, gp, 1, self.stride, (0, 0))
        else:
            addend = gp
        return self.conv1.dgrad(x.shape, gp1, residual=addend, mask_ref=x if mask_input else None, **kw)


class BlockStack:
    """resnet_utils.stack_blocks_dense (slim/nets/resnet_utils.py:126-200) for a list of
    (scope, depth, depth_bottleneck, stride-of-last-unit, num_units, trainable)."""

    def __init__(self, ps, prefix, cin, blocks, output_stride=None, current_stride=1, weight_decay=0.0,
                 bn_trainable=False):
        self.units = []
        rate = 1
        for (scope, base_depth, num_units, stride, trainable) in blocks:
            for i in range(num_units):
                ustride = stride if i == num_units - 1 else 1
                name = "%s/%s/unit_%d" % (prefix, scope, i + 1)
                if output_stride is not None and current_stride == output_stride:
                    u = Bottleneck(ps, name, cin, base_depth * 4, base_depth, 1, rate, trainable, weight_decay, bn_trainable)
                    rate *= ustride
                else:
                    u = Bottleneck(ps, name, cin, base_depth * 4, base_depth, ustride, 1, trainable, weight_decay,
                                   bn_trainable)
                    current_stride *= ustride
                u.block = scope
                self.units.append(u)
                cin = base_depth * 4
        self.cout = cin

    def layers(self):
        return [l for u in self.units for l in u.layers()]


class Tower:
    """The second-stage feature extractor, on RoI crops (under R-FCN: on the whole map) — DESIGN.md §1.1. A subclass
    sets `cout`, `trainable` and `out_act`, and has layers() -> [Layer] and forward(crops, save) -> (out, ctx)."""
    supports_wgrad_stream = False     # False: backward runs its filter gradients inline whatever `wgrad` it is given
    # out_act: the activation `out` went through, 'relu' | 'relu6', or None when it is not an activation of the tower's

    @staticmethod
    def out_hw(p):
        """Spatial size of the output for p x p crops."""
        return (p, p)

    @classmethod
    def out_mask(cls, feat):
        """mask_ref / mask6 of a predictor's backward for the features `feat` the tower produced: the tower's output
        activation fused into the gradient. Without one (`out_act` None) the gradient passes unmasked, through the exact
        zeros of the output too."""
        return dict(mask_ref=None if cls.out_act is None else feat, mask6=cls.out_act == "relu6")

    def backward(self, g_out, out, ctx, need_input_grad, masked=False, wgrad=INLINE_WGRAD, active=None):
        """g_out: dL/d(out), or dL/d(pre-activation of out) when `masked`. Returns dL/d(crops) or None.
        `wgrad`: where the filter gradients may run (inline, or a WgradStream the caller joins).
        active: uint8 flag per RoI, 0 = g_out is exactly zero there; a tower may use it to leave those RoIs' rows out of
        its GEMMs (same bits) or ignore it."""
        raise NotImplementedError


class FeatureExtractor:
    """The first-stage trunk and the factory of its towers — DESIGN.md §1.1. A subclass sets `cout` and `out_act` (the
    activation of the RPN feature map: 'relu' | 'relu6') and has layers(), preprocess(),
    extract_proposal_features(x, save) -> (features, ctx) and box_classifier_tower(scope, trainable) -> Tower."""
    supports_wgrad_stream = False     # as Tower's, for backward_proposal_features
    supports_rfcn = True              # False: RFCNMetaArch refuses the extractor
    min_image_size = 33               # None: the extractor takes any image size
    _neg_one = None

    def __init__(self, ps, is_training, first_stage_features_stride, weight_decay):
        if first_stage_features_stride not in (8, 16):
            raise ValueError("`first_stage_features_stride` must be 8 or 16.")
        self.ps, self.is_training, self.weight_decay = ps, is_training, weight_decay

    def check_inputs(self, x):
        if x.dim() != 4:
            raise ValueError("`preprocessed_inputs` must be 4 dimensional, got a tensor of shape %s" % (tuple(x.shape),))
        m = self.min_image_size
        if m is not None and (x.shape[1] < m or x.shape[2] < m):
            raise ValueError("image size must at least be %d in both height and width." % m)

    def to_unit_range(self, resized_inputs):
        """Maps pixel values to [-1, 1]: the preprocess of the MobileNet and Inception-ResNet-v2 extractors."""
        x = torch.empty_like(resized_inputs)
        ops.axpby(resized_inputs, x, 2.0 / 255.0, 0.0)
        if self._neg_one is None:
            self._neg_one = torch.full((3,), -1.0, dtype=torch.float32, device=x.device)
        return ops.bias_add_channels(x, self._neg_one)

    def backward_proposal_features(self, gp, ctx, wgrad=INLINE_WGRAD):
        """gp: dL/d(pre-activation of the RPN feature map) (already masked by `out_act`). `wgrad`: as Tower.backward's."""
        raise NotImplementedError
