"""MI355X-native drop-in for the reference's ``pointnet/PointNet.py``.

Same public names, constructor arguments, method names and layer names as
``/root/reference/point_cloud_analysis/pointnet/PointNet.py`` (PointNet :84-376, TNet :379-490,
ConvLayer :493-594, DenseLayer :597-679, PointCloudNormalization :681-712), but the arithmetic runs in
``libpointnet_hip.so`` (hand-written HIP for gfx950) on PyTorch-ROCm tensors.

There is NO CPU compute path: calling a model whose parameters are not on a HIP device raises
``PointNetHipError``.  Construction, freeze/thaw, ``get_layer_trainability``, ``get_config`` and weight
access are host logic and work anywhere.

Deviations from the reference, on purpose ("tolerate, not replicate"):
  * ``get_config`` includes ``vanilla`` (the reference omits it, PointNet.py:354-362, so a reloaded
    vanilla model silently became non-vanilla);
  * ``freeze_shared_network`` / ``thaw_shared_network`` work for ``vanilla=True`` (the reference
    dereferences ``None``, PointNet.py:302-318);
  * ``get_last_predicted_dcm`` returns the last predicted input transform (the reference calls a method
    its TNet does not define, PointNet.py:375-376);
  * reduce_max sends the gradient to the lowest-index maximum instead of splitting it among ties
    (identical parameter gradients when ties are duplicated points).
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import _lib
from .._lib import PointNetHipError, check, current_stream, lib, pn_model_desc, pn_model_io, pn_slot_info, ptr

BN_MOMENTUM = 0.99
BN_EPS = 1e-3


def _glorot_uniform(shape, seed: Optional[int]) -> torch.Tensor:
    """keras.initializers.GlorotUniform(seed).  As in the reference every seeded layer builds its own
    initializer from the SAME seed (PointNet.py:532,627,415), so same-shape layers start identical."""
    gen = torch.Generator()
    if isinstance(seed, int):
        gen.manual_seed(seed)
    else:
        gen.seed()
    fan_in, fan_out = shape[0], shape[1]
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return (torch.rand(shape, generator=gen, dtype=torch.float32) * 2 - 1) * lim


class _Weights:
    """Named views into the model's flat parameter buffer (layout defined by the C library)."""

    def __init__(self, desc: pn_model_desc, device):
        l = lib()
        n = l.pn_model_num_slots(C.byref(desc))
        if n <= 0:
            raise PointNetHipError("bad model descriptor: " + l.pn_last_error().decode())
        total = l.pn_model_param_floats(C.byref(desc))
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        self.slots: "OrderedDict[str, dict]" = OrderedDict()
        info = pn_slot_info()
        for i in range(n):
            check(l.pn_model_slot_info(C.byref(desc), i, C.byref(info)), "pn_model_slot_info")
            self.slots[info.name.decode()] = dict(offset=info.offset, rows=info.rows, cols=info.cols, kind=info.kind,
                                                  block=info.block)

    def view(self, name: str, flat: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self.slots[name]
        f = self.flat if flat is None else flat
        v = f[s["offset"]: s["offset"] + s["rows"] * s["cols"]]
        if s["kind"] in (0, 6, 7):
            return v.view(s["rows"], s["cols"])
        return v.view(s["cols"])


class _LayerBase:
    """Common freeze/thaw/name plumbing of the reference's custom layers."""

    def __init__(self, name: str):
        self.name = name
        self.trainable = True
        self._owner = None     # PointNet that owns the weights (None for a free-standing layer)
        self._prefix = None

    def is_trainable(self):
        return self.trainable

    def freeze(self):
        self.trainable = False

    def thaw(self):
        self.trainable = True

    def _w(self, suffix):
        if self._owner is None:
            own = getattr(self, "_own", None)
            if own is None or suffix not in own:
                raise PointNetHipError(f"layer {self.name} is not built")
            return own[suffix]
        return self._owner._weights.view(f"{self._prefix}.{suffix}")

    # ---- free-standing use (a layer that is not part of a PointNet owns its tensors) ----
    def _own_bn(self, width, device):
        self._own.update({"bn.gamma": torch.ones(width, device=device), "bn.beta": torch.zeros(width, device=device),
                          "bn.moving_mean": torch.zeros(width, device=device), "bn.moving_var": torch.ones(width, device=device)})

    @staticmethod
    def _device_of(x):
        _lib.require_gpu_tensor(x, "input", torch.float32)
        return x.device


class _BN:
    def __init__(self, layer, momentum):
        self._layer = layer
        self.momentum = momentum
        self.epsilon = BN_EPS
        self.trainable = True

    gamma = property(lambda self: self._layer._w("bn.gamma"))
    beta = property(lambda self: self._layer._w("bn.beta"))
    moving_mean = property(lambda self: self._layer._w("bn.moving_mean"))
    moving_variance = property(lambda self: self._layer._w("bn.moving_var"))


class ConvLayer(_LayerBase):
    """1x1 Conv2D (+BatchNormalization) (+activation) -- reference PointNet.py:493-594.  Inside a PointNet the
    layer is executed by the fused plan; free-standing use goes through ``pointcloudprocessing_amd.ops``."""

    def __init__(self, filters: int, name: str, kernel_size: tuple = (1, 1), strides: tuple = (1, 1), padding: str = 'same',
                 activation=None, apply_bn: bool = True, bn_momentum: float = 0.99, random_seed=None, **kwargs):
        super().__init__(f"{name}_convolution_layer")
        if tuple(kernel_size) != (1, 1) or tuple(strides) != (1, 1):
            raise PointNetHipError("only the 1x1 / stride-1 convolution the reference model uses is implemented")
        self.filters = filters
        self.kernel_size = tuple(kernel_size)
        self.strides = tuple(strides)
        self.padding = padding
        self.activation = activation
        self.apply_bn = apply_bn
        self.bn_momentum = bn_momentum
        self.seed = random_seed
        self.bn = _BN(self, bn_momentum) if apply_bn else None

    kernel = property(lambda self: self._w("kernel"))
    bias = property(lambda self: None if self.apply_bn else self._w("bias"))

    def freeze(self):
        self.trainable = False
        if self.apply_bn:
            self.bn.trainable = False

    def thaw(self):
        self.trainable = True
        if self.apply_bn:
            self.bn.trainable = True

    def build(self, input_shape, device="cuda"):
        """free-standing layer: Keras-style lazy weights (GlorotUniform kernel; BN gamma 1, beta 0, moving 0 / 1) -- PointNet.py:526-542"""
        cin = int(input_shape[-1])
        self._own = {"kernel": _glorot_uniform((cin, self.filters), self.seed).to(device)}
        if self.apply_bn:
            self._own_bn(self.filters, device)
        else:
            self._own["bias"] = torch.zeros(self.filters, device=device)

    def __call__(self, inputs, training: bool = False):
        """(B, N, 1, Cin) or (B, N, Cin) -> same rank with ``filters`` channels: Conv2D 1x1 -> BatchNormalization -> activation
        (PointNet.py:554-566), forward only, through the op-level C ABI (pn_conv_fwd / pn_conv3_fwd, pn_bn_finalize)."""
        from .. import ops
        if self._owner is not None:
            raise PointNetHipError("a layer inside a PointNet is executed by the model's plan; call the model")
        dev = self._device_of(inputs)
        if getattr(self, "_own", None) is None:
            self.build(inputs.shape, dev)
        shape = inputs.shape
        B, N, cin = shape[0], shape[1], shape[-1]
        x = inputs.reshape(B * N, cin).contiguous()
        w = self.kernel
        if cin == 3:
            z, part = ops.conv3_fwd(x, w, B, N)
        elif cin % 64 == 0 and self.filters % 64 == 0:
            z, part = ops.conv_fwd(_lib.operand(x, ld=cin), w, B, N, cin, self.filters, _lib.PN_PREC_BF16X3)
        else:
            raise PointNetHipError(f"ConvLayer: channel widths must be 3 or multiples of 64 (got {cin} -> {self.filters})")
        if self.apply_bn:
            batch = bool(training) and self.bn.trainable          # a frozen BN runs in inference mode (PointNet.py:585-591)
            _, _, scale, shift = ops.bn_finalize(part if batch else None, B * N, self.bn.gamma, self.bn.beta, self.bn.moving_mean,
                                                 self.bn.moving_variance, use_batch_stats=batch, update_moving=batch,
                                                 momentum=self.bn_momentum, eps=self.bn.epsilon)
            y = z * scale + shift
        else:
            y = z + self.bias
        if self.activation in ("relu", torch.relu) or getattr(self.activation, "__name__", "") == "relu":
            y = torch.relu(y)
        elif self.activation is not None:
            raise PointNetHipError(f"ConvLayer: activation {self.activation!r} is not implemented (the reference uses relu / None)")
        return y.reshape(*shape[:-1], self.filters)

    call = __call__

    def get_config(self):
        return {'filters': self.filters, 'name': self.name, 'kernel_size': self.kernel_size, 'strides': self.strides,
                'padding': self.padding, 'activation': self.activation, 'apply_bn': self.apply_bn,
                'bn_momentum': self.bn_momentum, 'random_seed': self.seed}


class DenseLayer(_LayerBase):
    """Dense (+BatchNormalization) (+activation) -- reference PointNet.py:597-679."""

    def __init__(self, units: int, name: str, activation=None, apply_bn: bool = False, bn_momentum: float = 0.99,
                 random_seed=None, **kwargs):
        super().__init__(f"{name}_dense_layer")
        self.units = units
        self.activation = activation
        self.apply_bn = apply_bn
        self.bn_momentum = bn_momentum
        self.seed = random_seed
        self.bn = _BN(self, bn_momentum) if apply_bn else None

    kernel = property(lambda self: self._w("kernel"))
    bias = property(lambda self: None if self.apply_bn else self._w("bias"))

    def freeze(self):
        self.trainable = False
        if self.apply_bn:
            self.bn.trainable = False

    def thaw(self):
        self.trainable = True
        if self.apply_bn:
            self.bn.trainable = True

    def build(self, input_shape, device="cuda"):
        cin = int(input_shape[-1])
        self._own = {"kernel": _glorot_uniform((cin, self.units), self.seed).to(device)}
        if self.apply_bn:
            self._own_bn(self.units, device)
        else:
            self._own["bias"] = torch.zeros(self.units, device=device)

    def __call__(self, inputs, training: bool = False):
        """(B, Cin) -> (B, units): Dense -> BatchNormalization -> activation (PointNet.py:642-654) in one native launch (pn_dense_layer)"""
        from .. import ops
        if self._owner is not None:
            raise PointNetHipError("a layer inside a PointNet is executed by the model's plan; call the model")
        dev = self._device_of(inputs)
        if getattr(self, "_own", None) is None:
            self.build(inputs.shape, dev)
        relu = self.activation in ("relu", torch.relu) or getattr(self.activation, "__name__", "") == "relu"
        if self.activation is not None and not relu:
            raise PointNetHipError(f"DenseLayer: activation {self.activation!r} is not implemented (the reference uses relu / None)")
        x = inputs.reshape(inputs.shape[0], -1).contiguous()
        if self.apply_bn:
            mode = 1 if (training and self.bn.trainable) else 2
            _, a, _, _ = ops.dense_layer(x, self.kernel, gamma=self.bn.gamma, beta=self.bn.beta, moving_mean=self.bn.moving_mean,
                                         moving_var=self.bn.moving_variance, bn_mode=mode, act=int(relu), momentum=self.bn_momentum,
                                         eps=self.bn.epsilon)
        else:
            _, a, _, _ = ops.dense_layer(x, self.kernel, bias=self.bias, bn_mode=0, act=int(relu))
        return a

    call = __call__

    def get_config(self):
        return {'units': self.units, 'name': self.name, 'activation': self.activation, 'apply_bn': self.apply_bn,
                'bn_momentum': self.bn_momentum, 'random_seed': self.seed}


class TNet(_LayerBase):
    """Transform network -- reference PointNet.py:379-490: three ConvLayers, max over points, two DenseLayers,
    ``@ w + b`` reshaped to (K, K)."""

    def __init__(self, name: str, add_regularization: bool = False, bn_momentum: float = 0.99,
                 layer_widths: list = [64, 128, 1024, 512, 256], random_seed=None, **kwargs):
        super().__init__(name)
        if list(layer_widths) != [64, 128, 1024, 512, 256]:
            raise PointNetHipError("only the reference's layer widths [64,128,1024,512,256] are implemented")
        self.add_regularization = add_regularization
        self.bn_momentum = bn_momentum
        self.layer_widths = list(layer_widths)
        self.seed = random_seed
        relu = "relu"
        self.conv_layer_1 = ConvLayer(filters=64, activation=relu, bn_momentum=bn_momentum, name=f"{name}_convolution_layer_1",
                                      random_seed=self.seed)
        self.conv_layer_2 = ConvLayer(filters=128, activation=relu, bn_momentum=bn_momentum, name=f"{name}_convolution_layer_2",
                                      random_seed=self.seed)
        self.conv_layer_3 = ConvLayer(filters=1024, activation=relu, bn_momentum=bn_momentum, name=f"{name}_convolution_layer_3",
                                      random_seed=self.seed)
        self.dense_layer_1 = DenseLayer(units=512, activation=relu, apply_bn=True, bn_momentum=bn_momentum,
                                        name=f"{name}_dense_layer_1", random_seed=self.seed)
        self.dense_layer_2 = DenseLayer(units=256, activation=relu, apply_bn=True, bn_momentum=bn_momentum,
                                        name=f"{name}_dense_layer_2", random_seed=self.seed)
        self._last_predicted = None

    w = property(lambda self: self._w("w"))
    b = property(lambda self: self._w("b"))

    def _sub(self):
        return [self.conv_layer_1, self.conv_layer_2, self.conv_layer_3, self.dense_layer_1, self.dense_layer_2]

    def freeze(self):
        self.trainable = False
        for l in self._sub():
            l.freeze()

    def thaw(self):
        self.trainable = True
        for l in self._sub():
            l.thaw()

    def is_trainable(self):
        return all(l.is_trainable() for l in self._sub())

    def get_last_predicted_transformation(self):
        return self._last_predicted

    def build(self, input_shape, device="cuda"):
        """free-standing T-Net: w = zeros (256, K^2), b = identity (K, K) -- PointNet.py:412-416"""
        K = int(input_shape[-1])
        self._own = {"w": torch.zeros(256, K * K, device=device), "b": torch.eye(K, device=device)}

    def __call__(self, inputs, training: bool = False):
        """(B, N, K), K in {3, 64} -> (B, K, K): three ConvLayers, max over the points, two DenseLayers, ``@ w + b`` (PointNet.py:418-454).
        Forward only, layer by layer through the op-level C ABI; inside a PointNet the fused plan runs instead."""
        from .. import ops
        if self._owner is not None:
            raise PointNetHipError("a T-Net inside a PointNet is executed by the model's plan; call the model")
        dev = self._device_of(inputs)
        if getattr(self, "_own", None) is None:
            self.build(inputs.shape, dev)
        B, N, K = inputs.shape
        x = self.conv_layer_1(inputs, training)
        x = self.conv_layer_2(x, training)
        x = self.conv_layer_3(x, training)
        g = torch.amax(x, dim=1)                                   # tf.reduce_max(X, axis=1)
        g = self.dense_layer_1(g, training)
        g = self.dense_layer_2(g, training)
        _, out, _, _ = ops.dense_layer(g, self.w, bias=self.b.reshape(-1).contiguous(), bn_mode=0, act=0)
        R = out.reshape(B, K, K)
        self._last_predicted = R
        return R

    call = __call__

    def get_config(self):
        return {'name': self.name, 'add_regularization': self.add_regularization, 'bn_momentum': self.bn_momentum,
                'layer_widths': self.layer_widths, 'random_seed': self.seed}


class PointCloudNormalization(_LayerBase):
    """Centre on the centroid, scale by the max radius (clamped at 1e-7) -- reference PointNet.py:681-712.
    Returns ``(normalized, (centroid, scale))``."""

    def __init__(self, name: str = "point_cloud_normalization", **kwargs):
        super().__init__(name)

    def __call__(self, input):
        from .. import ops
        return ops.normalize(input)

    call = __call__

    def is_trainable(self):
        return False

    def get_config(self):
        return {'name': self.name}


class _PointNetFn(torch.autograd.Function):
    """autograd bridge: forward = pn_model_forward, backward = pn_model_backward (whole model, native plan)."""

    @staticmethod
    def forward(ctx, flat, model, pc, training, fused):
        outs = model._run_forward(pc, training, fused)
        ctx.model = model
        ctx.training = training
        return outs

    @staticmethod
    def backward(ctx, d_cls, d_seg, d_R):
        model = ctx.model
        if not ctx.training:
            raise PointNetHipError("backward through a PointNet call made with training=False")
        g = model._run_backward(d_cls, d_seg, d_R)
        return g, None, None, None, None


def _scatter_rows(full_len, rows, value, fill):
    """(1, len(rows)) -> (1, full_len): ``value`` at ``rows``, ``fill`` on the rows predict_scan / predict_pose dropped"""
    out = torch.full((1, full_len), fill, device=value.device, dtype=value.dtype)
    out[0, rows] = value[0]
    return out


class PointNet(torch.nn.Module):
    """PointNet with classification, per-point segmentation and input-transform outputs
    (reference PointNet.py:84-376).  ``model(pc, training=...)`` returns ``[cls (B,Ccls), seg (B,N,Cseg), R (B,3,3)]``."""

    def __init__(self, classification_output_width: int, segmentation_output_width: int, dropout_rate: float,
                 random_seed: int, debugging: bool = False, vanilla: bool = False,
                 regularize_input_transform: bool = False, regularize_feature_transform: bool = False,
                 precision: str = "bf16x3", device=None, sync_bn_world: int = 1, sync_bn_rank: int = 0, sync_bn_group=None, **kwargs):
        """``sync_bn_world`` > 1 (data parallel, numerics-parity mode): every training-mode BatchNormalization takes its statistics over
        the clouds of ALL ranks, as the reference does on its one device (PointNet.py:528,559,623,647) -- a step on W ranks of B clouds
        is then the reference's step on the B*W clouds.  The collectives go through ``torch.distributed`` (``sync_bn_group`` or the
        default group); see include/pointnet_hip.h (pn_model_io.sync_hook) for what is exchanged and engine.TrainStep for the step."""
        super().__init__()
        self._classification_output_width = classification_output_width
        self._segmentation_output_width = segmentation_output_width
        self._dropout_rate = dropout_rate
        self._random_seed = random_seed
        self._debugging = debugging
        self._vanilla = vanilla
        self._regularize_input_transform = regularize_input_transform
        self._regularize_feature_transform = regularize_feature_transform
        if precision not in _lib.PREC:
            raise PointNetHipError(f"precision must be one of {list(_lib.PREC)}")
        self._precision = precision
        self._sync_world = int(sync_bn_world) if sync_bn_world and int(sync_bn_world) > 1 else 1
        self._sync_rank = int(sync_bn_rank) if self._sync_world > 1 else 0
        self._sync_group = sync_bn_group
        self._sync_error = None
        self._custom_layers = []
        self.input_names = ['pointnet_input']
        self.output_names = ['classification_output', 'segmentation_output', 'se3']

        relu, softmax = "relu", "softmax"
        seed = self._random_seed
        self.normalize_input = PointCloudNormalization(name="input_normalization")
        self.input_transform = TNet(name='input_transform', add_regularization=regularize_input_transform,
                                    random_seed=seed) if not vanilla else None
        self.mlp_1_1 = ConvLayer(filters=64, name='s1_l1_64', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_1_2 = ConvLayer(filters=64, name='s1_l2_64', activation=relu, apply_bn=True, random_seed=seed)
        self.feature_transform = TNet(name='feature_transform', add_regularization=regularize_feature_transform,
                                      random_seed=seed) if not vanilla else None
        self.mlp_2_1 = ConvLayer(filters=64, name='s2_l1_64', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_2_2 = ConvLayer(filters=128, name='s2_l2_128', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_2_3 = ConvLayer(filters=1024, name='s2_l3_1024', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_cls_1 = DenseLayer(units=512, name='s3_l1_512', activation=relu, apply_bn=True)
        self.mlp_cls_2 = DenseLayer(units=256, name='s3_l2_256', activation=relu, apply_bn=True)
        self.mlp_cls_3 = DenseLayer(units=classification_output_width, name='output', activation=softmax)
        self.mlp_seg_1 = ConvLayer(filters=512, name='seg_l1_512', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_seg_2 = ConvLayer(filters=256, name='seg_l2_256', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_seg_3 = ConvLayer(filters=128, name='seg_l3_128', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_seg_4 = ConvLayer(filters=128, name='seg_l4_128', activation=relu, apply_bn=True, random_seed=seed)
        self.mlp_seg_5 = ConvLayer(filters=segmentation_output_width, name='seg_l5_output', activation=softmax, apply_bn=False,
                                   random_seed=seed)

        self._custom_layers.append(self.normalize_input)
        if not vanilla:
            self._custom_layers.append(self.input_transform)
        self._custom_layers += [self.mlp_1_1, self.mlp_1_2]
        if not vanilla:
            self._custom_layers.append(self.feature_transform)
        self._custom_layers += [self.mlp_2_1, self.mlp_2_2, self.mlp_2_3, self.mlp_cls_1, self.mlp_cls_2, self.mlp_cls_3,
                                self.mlp_seg_1, self.mlp_seg_2, self.mlp_seg_3, self.mlp_seg_4, self.mlp_seg_5]

        # ---- weights: one flat buffer whose layout the C library defines ----
        self._desc = pn_model_desc(ccls=classification_output_width, cseg=segmentation_output_width, vanilla=int(vanilla),
                                   reg_in=int(regularize_input_transform), reg_feat=int(regularize_feature_transform),
                                   prec=_lib.PREC[precision], dropout_rate=float(dropout_rate), bn_momentum=BN_MOMENTUM,
                                   bn_eps=BN_EPS, sync_world=self._sync_world if self._sync_world > 1 else 0)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self._weights = _Weights(self._desc, torch.device(device))
        self.params_flat = torch.nn.Parameter(self._weights.flat)
        self._weights.flat = self.params_flat.data
        self.grads_flat = torch.zeros_like(self._weights.flat)
        self._bind_layers()
        self._initialize_weights()
        self._ws: Dict[tuple, torch.Tensor] = {}
        self._last = None
        self._built = False
        self.scalars = torch.zeros(16, dtype=torch.float32, device=self._weights.flat.device)
        self._fused_targets = None

    # ------------------------------------------------------------------ construction helpers
    def _bind_layers(self):
        def bind(layer, prefix):
            layer._owner, layer._prefix = self, prefix
        if not self._vanilla:
            for tn, pref in ((self.input_transform, "input_transform"), (self.feature_transform, "feature_transform")):
                bind(tn, pref)
                bind(tn.conv_layer_1, f"{pref}.conv1")
                bind(tn.conv_layer_2, f"{pref}.conv2")
                bind(tn.conv_layer_3, f"{pref}.conv3")
                bind(tn.dense_layer_1, f"{pref}.dense1")
                bind(tn.dense_layer_2, f"{pref}.dense2")
        for attr in ("mlp_1_1", "mlp_1_2", "mlp_2_1", "mlp_2_2", "mlp_2_3", "mlp_cls_1", "mlp_cls_2", "mlp_cls_3", "mlp_seg_1",
                     "mlp_seg_2", "mlp_seg_3", "mlp_seg_4", "mlp_seg_5"):
            bind(getattr(self, attr), attr)

    def _initialize_weights(self):
        W = self._weights
        seeded = {"mlp_cls_1", "mlp_cls_2", "mlp_cls_3"}       # the classification DenseLayers are unseeded (PointNet.py:130-134)
        with torch.no_grad():
            for name, s in W.slots.items():
                v = W.view(name)
                k = s["kind"]
                if k == 0 or k == 6:
                    seed = None if name.split(".")[0] in seeded else self._random_seed
                    v.copy_(_glorot_uniform((s["rows"], s["cols"]), seed))
                elif k == 1 or k == 4:
                    v.fill_(1.0)                                # gamma, moving_variance
                elif k == 7:
                    v.copy_(torch.eye(s["rows"]))               # T-Net b: 'identity' (PointNet.py:416)
                else:
                    v.zero_()                                   # beta, moving_mean, bias

    def build(self, input_shape):
        """Keras-style build; weights already exist, this only validates the shape (PointNet.py:161-195)."""
        if len(input_shape) != 3 or input_shape[2] != 3:
            raise PointNetHipError(f"PointNet expects (None, N, 3) inputs, got {input_shape}")
        self._built = True

    # ------------------------------------------------------------------ weights access
    def named_weights(self) -> "OrderedDict[str, torch.Tensor]":
        """name -> view into the flat buffer.  Names: '<block>[.<sub>].kernel|bn.gamma|bn.beta|bn.moving_mean|
        bn.moving_var|bias', '<tnet>.w', '<tnet>.b'; kernels are (Cin, Cout) like Keras."""
        return OrderedDict((n, self._weights.view(n)) for n in self._weights.slots)

    def named_grads(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((n, self._weights.view(n, self.grads_flat)) for n in self._weights.slots)

    def set_weights(self, weights: Dict[str, torch.Tensor]):
        with torch.no_grad():
            for n, t in weights.items():
                self._weights.view(n).copy_(torch.as_tensor(t, dtype=torch.float32).reshape(self._weights.view(n).shape))

    def count_params(self):
        tr = sum(s["rows"] * s["cols"] for s in self._weights.slots.values() if s["kind"] not in (3, 4))
        nt = sum(s["rows"] * s["cols"] for s in self._weights.slots.values() if s["kind"] in (3, 4))
        return tr, nt

    def trainable_mask(self) -> torch.Tensor:
        """1.0 where a flat-buffer element belongs to a trainable weight of a trainable block."""
        flags = self._block_flags()
        m = torch.zeros_like(self._weights.flat)
        for s in self._weights.slots.values():
            if s["kind"] not in (3, 4) and flags[s["block"]]:
                m[s["offset"]: s["offset"] + s["rows"] * s["cols"]] = 1.0
        return m

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._weights.flat = self.params_flat.data
        self.grads_flat = fn(self.grads_flat)
        self.scalars = fn(self.scalars)
        self._ws = {}
        return r

    # ------------------------------------------------------------------ trainability (PointNet.py:294-349)
    def _block_layers(self):
        return [self.input_transform, self.mlp_1_1, self.mlp_1_2, self.feature_transform, self.mlp_2_1, self.mlp_2_2, self.mlp_2_3,
                self.mlp_cls_1, self.mlp_cls_2, self.mlp_cls_3, self.mlp_seg_1, self.mlp_seg_2, self.mlp_seg_3, self.mlp_seg_4,
                self.mlp_seg_5]

    def _block_flags(self) -> List[int]:
        return [int(l.is_trainable()) if l is not None else 0 for l in self._block_layers()]

    def freeze_input_transform(self) -> None:
        if self._vanilla:
            print("PointNet:  No input transorm available to freeze.")
        else:
            self.input_transform.freeze()

    def thaw_input_transform(self) -> None:
        if self._vanilla:
            print("PointNet:  No input transorm available to thaw.")
        else:
            self.input_transform.thaw()

    def _shared(self):
        return [l for l in (self.input_transform, self.mlp_1_1, self.mlp_1_2, self.feature_transform, self.mlp_2_1, self.mlp_2_2,
                            self.mlp_2_3) if l is not None]

    def freeze_shared_network(self) -> None:
        for l in self._shared():
            l.freeze()

    def thaw_shared_network(self) -> None:
        for l in self._shared():
            l.thaw()

    def freeze_segmentation_head(self) -> None:
        for l in (self.mlp_seg_1, self.mlp_seg_2, self.mlp_seg_3, self.mlp_seg_4, self.mlp_seg_5):
            l.freeze()

    def thaw_segmentation_head(self) -> None:
        for l in (self.mlp_seg_1, self.mlp_seg_2, self.mlp_seg_3, self.mlp_seg_4, self.mlp_seg_5):
            l.thaw()

    def freeze_classification_head(self) -> None:
        for l in (self.mlp_cls_1, self.mlp_cls_2, self.mlp_cls_3):
            l.freeze()

    def thaw_classification_head(self) -> None:
        for l in (self.mlp_cls_1, self.mlp_cls_2, self.mlp_cls_3):
            l.thaw()

    def get_layer_trainability(self) -> dict:
        return {layer_.name: layer_.is_trainable() for layer_ in self._custom_layers}

    def get_config(self):
        return {'classification_output_width': self._classification_output_width,
                'segmentation_output_width': self._segmentation_output_width, 'dropout_rate': self._dropout_rate,
                'random_seed': self._random_seed, 'debugging': self._debugging, 'vanilla': self._vanilla,
                'regularize_input_transform': self._regularize_input_transform,
                'regularize_feature_transform': self._regularize_feature_transform, 'precision': self._precision}

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def get_last_predicted_dcm(self):
        return None if self._last is None else self._last[2]

    # ------------------------------------------------------------------ execution
    def _workspace(self, B, N, training):
        key = (B, N, bool(training))
        ws = self._ws.get(key)
        if ws is None:
            nbytes = lib().pn_model_workspace_bytes(C.byref(self._desc), B, N, int(training))
            if nbytes == 0:
                raise PointNetHipError("pn_model_workspace_bytes failed: " + lib().pn_last_error().decode())
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self._weights.flat.device)
            self._ws[key] = ws
        return ws

    @property
    def activation_dtype(self):
        """storage type of the per-point layer-boundary tensors of the plan (workspace entries *.Z, *.dy, *.D, X64, dX64, tmpA12)"""
        return torch.bfloat16 if self._desc.prec & _lib.PN_STORE_BF16 else torch.float32

    def workspace_tensor(self, name: str, B: int, N: int, training: bool, dtype=torch.float32) -> torch.Tensor:
        """View of a named intermediate of the last call of that shape (test introspection)."""
        off, nb = C.c_int64(), C.c_int64()
        check(lib().pn_model_ws_lookup(C.byref(self._desc), B, N, int(training), name.encode(), C.byref(off), C.byref(nb)),
              "pn_model_ws_lookup")
        return self._workspace(B, N, training)[off.value: off.value + nb.value].view(dtype)

    def _io(self, pc, training, fused):
        B, N, _ = pc.shape
        dev = pc.device
        ws = self._workspace(B, N, training)
        io = pn_model_io()
        io.pc = pc.data_ptr()
        io.B, io.N = B, N
        io.params = self._weights.flat.data_ptr()
        io.grads = self.grads_flat.data_ptr() if training else None
        self._flags_c = (C.c_uint8 * _lib.PN_NUM_BLOCKS)(*self._block_flags())
        io.trainable = C.cast(self._flags_c, C.c_void_p)
        io.training = int(training)
        io.workspace = ws.data_ptr()
        io.workspace_bytes = ws.numel()
        if self._debugging or getattr(self, "keep_activations", False):      # check_numerics reads every layer's stored output
            io.flags = _lib.PN_IO_KEEP_ACTIVATIONS
        io.scalars = self.scalars.data_ptr()
        aux = getattr(self, "_aux_stream", None)       # engine.TrainStep: parameter gradients on a second stream
        io.aux_stream = aux.cuda_stream if (aux is not None and training) else None
        keep = None
        W = self._sync_world if training else 1
        if W > 1:
            io.sync_rank = self._sync_rank
            io.sync_hook = C.cast(self._sync_hook_c(), C.c_void_p)
            self._sync_ws = ws
        if training and self._dropout_rate > 0:
            if fused is not None and fused.get("keep") is not None:
                keep = fused["keep"]
                if keep[0].numel() != B * W * 512 or keep[1].numel() != B * W * 256:
                    raise PointNetHipError(f"dropout keep masks need {B * W} rows (synchronised BatchNormalization: the rows of all ranks)")
            else:
                if W > 1:
                    raise PointNetHipError("synchronised BatchNormalization needs the dropout keep masks of all ranks' rows (engine.TrainStep draws them)")
                keep = ((torch.rand(B, 512, device=dev) >= self._dropout_rate).to(torch.uint8),
                        (torch.rand(B, 256, device=dev) >= self._dropout_rate).to(torch.uint8))
            io.keep1, io.keep2 = keep[0].data_ptr(), keep[1].data_ptr()
            rng = None if fused is None else fused.get("dropout_rng")
            if rng is not None:        # (seed, device uint32 step counter): the forward's first launch draws the masks into `keep`
                io.dropout_seed, io.dropout_step = int(rng[0]), rng[1].data_ptr()
        if fused is not None and fused.get("zero_grads_in_forward"):
            io.zero_grads_in_forward = 1
        if fused is not None and fused.get("labels_cls") is not None:
            _lib.require_gpu_tensor(fused["labels_cls"], "labels_cls", torch.int32)
            _lib.require_gpu_tensor(fused["labels_seg"], "labels_seg", torch.int32)
            _lib.require_gpu_tensor(fused["se3"], "se3", torch.float32)
            if fused["labels_cls"].numel() != B or fused["labels_seg"].numel() != B * N or fused["se3"].numel() != B * 9:
                raise PointNetHipError("fused loss targets have the wrong number of elements")
            io.labels_cls = fused["labels_cls"].data_ptr()
            io.labels_seg = fused["labels_seg"].data_ptr()
            io.se3 = fused["se3"].data_ptr()
            lw = fused["loss_weights"]
            # synchronised BatchNormalization: every rank seeds the gradient of the GLOBAL mean loss (pn_model_io.sync_hook)
            io.loss_weights[0], io.loss_weights[1], io.loss_weights[2] = float(lw[0]) / W, float(lw[1]) / W, float(lw[2]) / W
        return io, keep

    # ------------------------------------------------------------------ synchronised BatchNormalization
    def _sync_hook_c(self):
        """the C callback the native plan calls between two of its launches (pn_model_io.sync_hook): op 0 all-reduce (sum), op 1 all-gather,
        on ranges of the workspace, through torch.distributed on the current stream"""
        if getattr(self, "_sync_cb", None) is None:
            import torch.distributed as dist

            def hook(ctx, op, src, dst, n, dtype, stream):
                try:
                    ws = self._sync_ws
                    base, es = ws.data_ptr(), (4 if dtype == 0 else 8)
                    tdt = torch.float32 if dtype == 0 else torch.int64

                    def view(ptr_, count):
                        off = ptr_ - base
                        if off < 0 or off + count * es > ws.numel():
                            raise PointNetHipError("sync_hook: range outside the workspace")
                        return ws[off: off + count * es].view(tdt)
                    W = self._sync_world
                    if op == 0:
                        d = view(dst, n)
                        if src != dst:
                            d.copy_(view(src, n))
                        dist.all_reduce(d, group=self._sync_group)
                    else:
                        out, mine = view(dst, n * W), view(src, n).clone()
                        dist.all_gather([out[i * n:(i + 1) * n] for i in range(W)], mine, group=self._sync_group)
                    return 0
                except Exception as e:      # never let an exception cross the C frame
                    self._sync_error = f"{type(e).__name__}: {e}"
                    return 1
            self._sync_cb = _lib.SYNC_HOOK(hook)
        return self._sync_cb

    def replicated_grad_mask(self) -> torch.Tensor:
        """synchronised BatchNormalization: 0.0 where every rank computes a gradient slot IN FULL (all bn.gamma / bn.beta -- formed from
        the sums over all ranks; the per-cloud dense layers' kernels and bias and the T-Nets' w / b -- run on all ranks' rows), 1.0 where
        a rank holds its clouds' share.  Every rank but one multiplies its gradients by this before they are summed."""
        m = torch.ones_like(self._weights.flat)
        dense_blocks = ("mlp_cls_1", "mlp_cls_2", "mlp_cls_3")
        for name, s in self._weights.slots.items():
            k = s["kind"]
            rep = k in (1, 2, 6, 7) or (k in (0, 5) and (name.split(".")[0] in dense_blocks or ".dense" in name))
            if rep:
                m[s["offset"]: s["offset"] + s["rows"] * s["cols"]] = 0.0
        return m

    def _run_forward(self, pc, training, fused):
        _lib.require_gpu_tensor(pc, "pc", torch.float32)
        if not self._weights.flat.is_cuda:
            raise PointNetHipError("PointNet parameters are not on a HIP device: there is no CPU compute path")
        if pc.dim() != 3 or pc.shape[2] != 3:
            raise PointNetHipError(f"PointNet expects (B, N, 3) inputs, got {tuple(pc.shape)}")
        B, N, _ = pc.shape
        dev = pc.device
        io, keep = self._io(pc, training, fused)
        cls = torch.empty(B, self._classification_output_width, device=dev, dtype=torch.float32)
        seg = torch.empty(B, N, self._segmentation_output_width, device=dev, dtype=torch.float32)
        R = torch.empty(B, 3, 3, device=dev, dtype=torch.float32)
        io.out_cls, io.out_seg, io.out_R = cls.data_ptr(), seg.data_ptr(), R.data_ptr()
        rc = lib().pn_model_forward(C.byref(self._desc), C.byref(io), current_stream())
        if rc != 0 and self._sync_error:
            raise PointNetHipError(f"pn_model_forward: collective failed inside sync_hook: {self._sync_error}")
        check(rc, "pn_model_forward")
        if self._debugging:
            self._check_numerics(pc, cls, seg, training)
        self._last = (cls, seg, R)
        self._last_call = dict(pc=pc, training=training, fused=fused, keep=keep, io=io)
        if not self._vanilla:
            self.input_transform._last_predicted = R
        return cls, seg, R

    def _check_numerics(self, pc, cls, seg, training):
        """``debugging: true`` (reference pointnet_train.py:112): PointNet.call wraps its input and every layer output in
        tf.debugging.check_numerics (PointNet.py:199-288).  The plan stores each ConvLayer's pre-BN output and BN coefficients, the
        pooled features and the head activations; they are scanned on the device (pn_count_nonfinite) in the reference's order and the
        first site holding a NaN / Inf raises with the reference's own message.  One host read per call: debug mode only, never inside
        a captured step."""
        B, N, _ = pc.shape
        def t(name, dtype=torch.float32):
            return self.workspace_tensor(name, B, N, training, dtype)
        act = self.activation_dtype
        conv = lambda wn: [t(wn + ".Z", act), t(wn + ".scale"), t(wn + ".shift")]          # noqa: E731
        sites = [("Input point cloud contains nan values", "pointnet_input", [pc])]
        if not self._vanilla:
            sites.append(("Input transform produced nan values.", self.input_transform.name, [t("iT.R"), t("Weff1")]))
        sites += [("mlp_1_1 produced nan values.", self.mlp_1_1.name, conv("m11")),
                  ("mlp_1_2 produced nan values.", self.mlp_1_2.name, conv("m12"))]
        if not self._vanilla:
            sites.append(("Feature transform produced nan values.", self.feature_transform.name, [t("fT.R"), t("X64", act)]))
        sites += [("mlp_2_1 produced nan values.", self.mlp_2_1.name, conv("m21")),
                  ("mlp_2_2 produced nan values.", self.mlp_2_2.name, conv("m22")),
                  ("mlp_2_3 produced nan values.", self.mlp_2_3.name, [t("mm23.zstar"), t("mm23.g")]),
                  ("mlp_cls_1 produced nan values.", self.mlp_cls_1.name, [t("c1.a")]),
                  ("mlp_cls_2 produced nan values.", self.mlp_cls_2.name, [t("c2.a")]),
                  ("mlp_cls_3 produced nan values.", self.mlp_cls_3.name, [cls]),
                  ("mlp_3_1 produced nan values.", self.mlp_seg_1.name, conv("s1")),
                  ("mlp_3_2 produced nan values.", self.mlp_seg_2.name, conv("s2")),
                  ("mlp_3_3 produced nan values.", self.mlp_seg_3.name, conv("s3")),
                  ("mlp_3_4 produced nan values.", self.mlp_seg_4.name, conv("s4")),
                  ("mlp_3_5 produced nan values.", self.mlp_seg_5.name, [seg])]
        counts = torch.zeros(len(sites), dtype=torch.int32, device=pc.device)
        for i, (_, _, tensors) in enumerate(sites):
            for x in tensors:
                check(lib().pn_count_nonfinite(ptr(x), x.numel(), int(x.dtype == torch.bfloat16), ptr(counts[i:i + 1]), current_stream()),
                      "pn_count_nonfinite")
        bad = counts.cpu().tolist()
        for (msg, layer, _), n in zip(sites, bad):
            if n:
                raise PointNetHipError(f"check_numerics: {msg} ({n} non-finite values at layer '{layer}')")

    def _run_backward(self, d_cls, d_seg, d_R, phase: int = 0):
        """phase 0: the whole backward pass; 1 / 2: its two halves (pn_model_io.bwd_phase) for gradient-bucket overlap"""
        lc = self._last_call
        io = lc["io"]
        io.bwd_phase = int(phase)
        def c(t):
            return None if t is None else t.contiguous()
        d_cls, d_seg, d_R = c(d_cls), c(d_seg), c(d_R)
        rc = lib().pn_model_backward(C.byref(self._desc), C.byref(io), ptr(d_cls), ptr(d_seg), ptr(d_R), current_stream())
        if rc != 0 and self._sync_error:
            raise PointNetHipError(f"pn_model_backward: collective failed inside sync_hook: {self._sync_error}")
        check(rc, "pn_model_backward")
        return self.grads_flat

    def forward(self, pc, training: Optional[bool] = None):
        training = self.training if training is None else bool(training)
        if training and torch.is_grad_enabled():
            outs = _PointNetFn.apply(self.params_flat, self, pc, True, None)
        else:
            outs = self._run_forward(pc, training, None)
        return [outs[0], outs[1], outs[2]]

    call = forward

    def predict(self, pc):
        """inference entry: ``(class index (B,), part index per point (B, N), R (B,3,3))`` -- the arg-max of the two softmax
        outputs (first maximum, np.argmax order), taken on the device (pn_argmax_rows).  Indices are int32."""
        from .. import ops
        cls, seg, R = self._run_forward(pc, False, None)
        return ops.argmax_rows(cls), ops.argmax_rows(seg), R

    def _kept_rows(self, xyz, denoise, isolate, cluster_leaf, min_cluster_points, remove_planes=None, cluster_density=None):
        """the rows (ascending: scan order) of the scan that predict_scan / predict_pose run on: first ``remove_planes`` (a dict of
        ops.plane_segment keywords) drops the floor and the walls -- a floor would give every stray near it neighbours enough to pass
        ``denoise`` -- then ``denoise`` (a dict of ops.outlier_mask keywords) drops the outliers, so that noise cannot bridge two
        bodies, then ``isolate="largest"`` keeps the largest voxel cluster of what is left at ``cluster_leaf`` (ops.voxel_clusters,
        26-connectivity), or, with ``cluster_density=dict(eps=, min_points=)``, the largest density cluster (ops.dbscan)"""
        from .. import ops
        if isolate is not None and isolate != "largest":
            raise PointNetHipError(f"isolate must be None or 'largest', got {isolate!r}")
        if cluster_density is not None:
            if not isinstance(cluster_density, dict) or set(cluster_density) != {"eps", "min_points"}:
                raise PointNetHipError(f"cluster_density must be None or dict(eps=..., min_points=...), got {cluster_density!r}")
            if isolate is None:
                raise PointNetHipError("cluster_density goes with isolate='largest'")
        _lib.require_gpu_tensor(xyz, "xyz", torch.float32)
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise PointNetHipError(f"predict_scan expects (N, 3) points, got {tuple(xyz.shape)}")
        rows = None
        if remove_planes is not None:
            if not isinstance(remove_planes, dict):
                raise PointNetHipError(f"remove_planes must be None or a dict of ops.plane_segment keywords, got {remove_planes!r}")
            rows = (ops.plane_mask(ops.plane_segment(xyz, **remove_planes)[2]) & torch.isfinite(xyz).all(1)).nonzero().squeeze(1)
            if rows.numel() == 0:
                raise PointNetHipError("remove_planes: no point of the scan was kept")
        if denoise is not None:
            if not isinstance(denoise, dict):
                raise PointNetHipError(f"denoise must be None or a dict of ops.outlier_mask keywords, got {denoise!r}")
            kept = ops.outlier_mask(xyz if rows is None else xyz[rows].contiguous(), **denoise).nonzero().squeeze(1)
            rows = kept if rows is None else rows[kept]
            if rows.numel() == 0:
                raise PointNetHipError("denoise: no point of the scan was kept")
        if isolate is None:
            return rows
        pts = xyz if rows is None else xyz[rows].contiguous()
        if cluster_density is not None:
            cluster, sizes = ops.dbscan(pts, cluster_density["eps"], cluster_density["min_points"])
        else:
            cluster, sizes = ops.voxel_clusters(pts, cluster_leaf)
        largest = int(sizes.max().item()) if sizes.numel() else 0
        if largest < max(int(min_cluster_points), 1):
            raise PointNetHipError(f"isolate: the largest cluster has {largest} points, fewer than min_cluster_points={min_cluster_points}")
        kept = ops.cluster_mask(cluster, sizes, "largest").nonzero().squeeze(1)
        return kept if rows is None else rows[kept]

    def predict_scan(self, xyz, leaf=0.25, samples: int = 8192, k: int = 3, origin=None, return_confidence: bool = False,
                     isolate=None, cluster_leaf=1.0, min_cluster_points: int = 1, denoise=None, remove_planes=None, cluster_density=None):
        """inference on a dense scan, a part index for EVERY scan point: xyz (N, 3) fp32 on the device -> voxel grid (``leaf``,
        ``origin``: default the scan's per-axis minimum) -> M = min(samples, V) centroids by FPS (start 0; all V centroids in voxel
        order when V <= samples) -> the forward pass on the sampled (1, M, 3) cloud -> every scan point takes the inverse-distance
        mix of the segmentation probabilities of its ``k`` nearest samples and the arg-max of that mix (ops.knn_propagate).
        Returns ``(class index (1,), part index per scan point (1, N), R (1, 3, 3))``, the convention of ``predict`` with B = 1.
        With ``return_confidence`` a fourth value follows: conf (1, N) fp32, the propagated mix's value at that arg-max (the
        probability the scan point's part got), 0 where the part is -1; ops.semantic_icp takes it as ``weights``.
        Inference only (moving BatchNormalization statistics, no dropout).  Host reads: the voxel count (it sizes the sampled
        cloud), and the per-axis minimum when ``origin`` is None.
        ``isolate="largest"`` first finds the object in a cluttered scan: the scan is clustered at ``cluster_leaf``
        (ops.voxel_clusters, 26-connectivity), the points of the largest cluster are compacted in scan order, the pipeline above runs
        on them alone (``origin=None``: their minimum) and the results are scattered back to full length: a dropped point (strays,
        ground returns, a second body, a non-finite row) gets part -1 and confidence 0; the shapes do not change.  Raises when the
        largest cluster has fewer than ``min_cluster_points`` points.  It adds the host reads of ops.voxel_clusters.
        ``cluster_density=dict(eps=..., min_points=...)`` (with ``isolate="largest"``) takes the clusters from ops.dbscan instead:
        exact DBSCAN, which a string of single returns between two bodies does not bridge and whose answer does not depend on where
        a grid falls; ``cluster_leaf`` is then unused, the noise points are dropped with the other clusters, and the host reads are
        those of ops.dbscan.  Without ``isolate``, or with other keys than ``eps`` and ``min_points``, it raises.
        ``denoise`` (a dict of ops.outlier_mask keywords, e.g. ``dict(method="radius", radius=1.5, min_neighbors=8)``) drops the
        scan's outliers (mixed pixels, dust, spray) through the same compact -> run -> scatter-back path, BEFORE ``isolate``: noise
        must not bridge two bodies.  A dropped point gets part -1 and confidence 0.  It adds the host reads of ops.radius_knn.
        ``dict(method="incidence", radius=0.6, k=8, max_angle_deg=75)`` is the mixed-pixel filter: it drops a point whose surface
        normal (ops.estimate_normals) is nearly perpendicular to its view ray -- the veil between a foreground edge and the surface
        close behind it, which is as dense as a surface and passes ``"radius"``.  Its ``viewpoint`` defaults to the sensor origin,
        (0, 0, 0): pass the sensor's position for a scan that is not in the sensor frame.
        ``remove_planes`` (a dict of ops.plane_segment keywords, e.g. ``dict(threshold=0.1, max_planes=2, min_inliers=2000)``) first
        drops the supporting surfaces -- the floor under the object, a wall behind it: dense and joined to the object, so neither
        ``denoise`` nor ``isolate`` can -- through the same path, BEFORE ``denoise`` and ``isolate``.  A point on a plane (and a
        non-finite row) gets part -1 and confidence 0.  Raises when nothing is kept.  It adds one host read, the kept rows."""
        from .. import ops
        if isolate is not None or denoise is not None or remove_planes is not None or cluster_density is not None:
            rows = self._kept_rows(xyz, denoise, isolate, cluster_leaf, min_cluster_points, remove_planes, cluster_density)
            outs = self.predict_scan(xyz[rows].contiguous(), leaf=leaf, samples=samples, k=k, origin=origin, return_confidence=return_confidence)
            part = _scatter_rows(xyz.shape[0], rows, outs[1], -1)
            if not return_confidence:
                return outs[0], part, outs[2]
            return outs[0], part, outs[2], _scatter_rows(xyz.shape[0], rows, outs[3], 0)
        _lib.require_gpu_tensor(xyz, "xyz", torch.float32)
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise PointNetHipError(f"predict_scan expects (N, 3) points, got {tuple(xyz.shape)}")
        if origin is None:
            origin = xyz.min(0).values.cpu().tolist()
        cent, _, _ = ops.voxel_downsample(xyz, ops._leaf3(leaf, "predict_scan"), origin)
        V = cent.shape[0]
        if V > samples:
            idx = ops.farthest_point_sample(cent.unsqueeze(0).contiguous(), int(samples))
            cloud = cent[idx[0].long()].unsqueeze(0).contiguous()
        else:
            cloud = cent.unsqueeze(0).contiguous()
        cls, seg, R = self._run_forward(cloud, False, None)
        _, _, mix, part = ops.knn_propagate(xyz.unsqueeze(0), cloud, k, values=seg)
        if not return_confidence:
            return ops.argmax_rows(cls), part, R
        conf = mix.gather(2, part.long().clamp(min=0).unsqueeze(2)).squeeze(2)
        return ops.argmax_rows(cls), part, R, torch.where(part >= 0, conf, torch.zeros_like(conf))

    def predict_pose(self, xyz, reference, leaf=0.25, samples: int = 8192, k: int = 3, init=None, origin=None, weights=None,
                     isolate=None, cluster_leaf=1.0, min_cluster_points: int = 1, denoise=None, remove_planes=None, cluster_density=None,
                     **icp):
        """6-DoF pose of a dense scan: ``predict_scan`` gives every scan point a part label, then the labelled ``reference``
        (ops.icp_reference, in this model's part-label space) is registered against the labelled scan by ops.semantic_icp.
        Initial pose: R is the input T-Net's matrix as returned by ``predict_scan`` (the model applies it as ``x = pcn @ R``,
        i.e. x = R^T p for column vectors, so p ~= R q maps the canonical frame to the scan: the pose convention
        p_scan ~= R q_ref + t), projected onto the nearest rotation; t = c_scan - R c_ref with both centroids over the points whose label is present in both clouds
        (all points when none is).  ``init`` (4, 4) or (1, 4, 4) overrides the initial pose; ``init="global"`` takes no start
        at all: the pose is what ops.global_pose returns (scored multi-start from the part labels, for a model whose T-Net
        carries no pose information; it needs a finite ``max_dist`` and also takes ``rotations``, ``top``, ``stride`` and, with a mesh reference, ``score_cloud``).  ``icp`` goes to
        ops.semantic_icp (max_iters, max_dist, tol_rot, tol_t, metric): ``metric="plane"`` registers point to plane against the
        reference's normals (``reference`` from ops.icp_normals, or ops.icp_reference(normals=...)), which converges in far
        fewer iterations on surface-sampled scans.  ``reference`` may also be an ops.IcpMeshReference (ops.icp_mesh_reference, e.g.
        from pointcloud.read_labelled_mesh): the scan is then registered point to triangle against the mesh, for either metric,
        with the face normals the mesh carries.  An ops.IcpGridReference (ops.icp_reference / ops.mesh_sample_reference with
        accel="grid", max_dist=...) is searched through its voxel grid and gives the pose of the plain reference bit for bit; it
        needs ``max_dist`` in ``icp``, at most the reference's, and takes no ``robust`` / ``weights``.  ``robust`` ("huber", "cauchy", "tukey", with robust_scale, robust_tune,
        robust_min_scale) and ``weights`` select ops.semantic_icp's robust, confidence-weighted loop, which a share of wrong part
        labels does not pull off the pose: ``weights="confidence"`` weights every scan point by the confidence of its label
        (``predict_scan(return_confidence=True)``), a (1, N) fp32 tensor is passed through; init="global" takes ``robust`` but no
        weights.  Returns ``(class index (1,), part (1, N), pose (1, 4, 4) fp64, rmse (1,),
        pairs (1,))``.  No host synchronisation beyond predict_scan's.
        ``isolate``, ``cluster_leaf``, ``min_cluster_points``, ``cluster_density``: as in ``predict_scan``.  Segmentation AND registration then run on the
        kept points alone (a (1, N) ``weights`` tensor is compacted with them), so the pose is the pose of the object's own scan
        bit for bit; ``part`` comes back at full length with -1 on the dropped points.  ``denoise``: as in ``predict_scan``, applied
        before ``isolate``, with the same compaction of points and weights (``method="incidence"``: the viewpoint defaults to the sensor
        origin).  ``remove_planes``: as in ``predict_scan``, applied first."""
        from .. import ops
        if isolate is not None or denoise is not None or remove_planes is not None or cluster_density is not None:
            rows = self._kept_rows(xyz, denoise, isolate, cluster_leaf, min_cluster_points, remove_planes, cluster_density)
            if isinstance(weights, torch.Tensor):
                weights = weights.reshape(1, -1)[:, rows].contiguous()
            ci, kept, pose, rmse, pairs = self.predict_pose(xyz[rows].contiguous(), reference, leaf=leaf, samples=samples, k=k, init=init,
                                                            origin=origin, weights=weights, **icp)
            return ci, _scatter_rows(xyz.shape[0], rows, kept, -1), pose, rmse, pairs
        if isinstance(weights, str):
            if weights != "confidence":
                raise PointNetHipError(f"predict_pose: weights must be None, a (1, N) tensor or 'confidence', got {weights!r}")
            ci, part, R, weights = self.predict_scan(xyz, leaf=leaf, samples=samples, k=k, origin=origin, return_confidence=True)
        else:
            ci, part, R = self.predict_scan(xyz, leaf=leaf, samples=samples, k=k, origin=origin)
        if weights is not None:
            icp["weights"] = weights
        if isinstance(init, str):
            if init != "global":
                raise PointNetHipError(f"predict_pose: init must be None, a (4, 4) pose or 'global', got {init!r}")
            if "max_dist" not in icp:
                raise PointNetHipError("predict_pose: init='global' needs a finite max_dist")
            pose, rmse, pairs, _, _, _, _ = ops.global_pose(xyz.unsqueeze(0), part, reference, **icp)
            return ci, part, pose, rmse, pairs
        if init is not None:
            pose0 = torch.as_tensor(init, dtype=torch.float64, device=xyz.device).reshape(1, 4, 4)
        else:
            pose0 = self.initial_pose(xyz, part, R, reference)
        pose, rmse, pairs, _, _ = ops.semantic_icp(xyz.unsqueeze(0), part, reference, pose0, **icp)
        return ci, part, pose, rmse, pairs

    @staticmethod
    def initial_pose(xyz, part, R, reference):
        """the starting pose of predict_pose (1, 4, 4) fp64: [Rn | c_scan - Rn c_ref] with Rn the rotation nearest to the T-Net's
        R (1, 3, 3) in the Frobenius norm, the centroids (fp64 torch reductions on the
        device) over the points whose label lies in [0, n_parts) and is present in both the scan's ``part`` (1, N) and the
        reference; over all points (labelled or not) when no label is shared.  With an ops.IcpMeshReference the reference
        centroid is the area-weighted mean of the triangle centroids over the same labels (all triangles when none is shared)."""
        from .. import ops
        dev = xyz.device
        n_parts = reference.n_parts
        seg = torch.tensor(reference.seg, device=dev)
        lab = part[0].long()
        valid = (lab >= 0) & (lab < n_parts)
        in_scan = torch.bincount(torch.where(valid, lab, n_parts), minlength=n_parts + 1)[:n_parts] > 0
        both = (seg[1:] > seg[:-1]) & in_scan
        ref_lab = torch.repeat_interleave(torch.arange(n_parts, device=dev), seg[1:] - seg[:-1], output_size=reference.M)
        any_both = both.any()
        use_s = torch.where(any_both, valid & both[lab.clamp(0, n_parts - 1)], torch.ones_like(valid)).double()
        use_r = torch.where(any_both, both[ref_lab], torch.ones_like(both[ref_lab])).double()
        c_scan = (xyz.double() * use_s[:, None]).sum(0) / use_s.sum()
        if isinstance(reference, ops.IcpMeshReference):
            # a mesh: the area-weighted mean of the triangle centroids (the centroid of the surface)
            wgt = use_r * reference.area.double()
            c_ref = (reference.tri.double().mean(1) * wgt[:, None]).sum(0) / wgt.sum()
        else:
            c_ref = (reference.xyz.double() * use_r[:, None]).sum(0) / use_r.sum()
        # the T-Net's matrix is only regularised towards orthogonality: start from the nearest rotation, the Kabsch solve of
        # sums whose centred cross-covariance is H = R^T (argmax over rotations X of trace(X R^T))
        S = torch.zeros(1, 18, dtype=torch.float64, device=dev)
        S[0, 0] = 3.0
        S[0, 7:16] = R[0].double().t().reshape(9)
        R64 = ops.icp_solve(S, torch.eye(4, dtype=torch.float64, device=dev).unsqueeze(0))[0][0, :3, :3]
        pose0 = torch.eye(4, dtype=torch.float64, device=dev)
        pose0[:3, :3] = R64
        pose0[:3, 3] = c_scan - R64 @ c_ref
        return pose0.unsqueeze(0)

    def grad_extent(self):
        """(lo, hi): the smallest range of ``grads_flat`` (floats) that holds every gradient of a trainable block.  Outside it the
        gradient is identically zero on every rank and every step (frozen blocks, PointNet.py:294-349): the data-parallel all-reduce
        and the optimizer skip it -- with fresh optimizer state (the trainer builds one per profile stage, pointnet_train.py:310-319)
        Adam's update of a zero-gradient element is exactly zero, so nothing changes but the bytes moved."""
        flags = self._block_flags()
        lo, hi = None, 0
        for s in self._weights.slots.values():
            if s["kind"] not in (3, 4) and flags[s["block"]]:
                o, e = int(s["offset"]), int(s["offset"]) + int(s["rows"]) * int(s["cols"])
                lo = o if lo is None else min(lo, o)
                hi = max(hi, e)
        if lo is None:
            return 0, 0
        return lo, (hi + 63) // 64 * 64 if (hi + 63) // 64 * 64 <= self.grads_flat.numel() else hi

    def grad_bucket_boundary(self) -> int:
        """offset (floats) in ``grads_flat`` from which every slot is final after backward phase 1"""
        for n, s in self._weights.slots.items():
            if n.startswith("feature_transform." if not self._vanilla else "mlp_2_1."):
                return int(s["offset"])
        raise PointNetHipError("parameter layout has no feature_transform / mlp_2_1 slot")

    def fused_loss_step(self, pc, labels_cls, labels_seg, se3, loss_weights, keep=None, backward_phase: int = 0, dropout_rng=None):
        """forward + the three keras losses of pointnet_train.py:334-345 + backward, all native.  Leaves the
        gradients in ``grads_flat`` and the loss / metric sums in ``self.scalars`` (see pn_model_io).
        ``keep``: the two dropout keep masks (uint8 tensors) -- inputs, or, with ``dropout_rng=(seed, step_counter_tensor)``, buffers
        the forward pass fills from its counter-based generator (pn_model_io.dropout_step)."""
        fused = dict(labels_cls=labels_cls, labels_seg=labels_seg.reshape(-1), se3=se3, loss_weights=loss_weights, keep=keep,
                     dropout_rng=dropout_rng, zero_grads_in_forward=True)      # the backward pass follows: one clearing launch less
        outs = self._run_forward(pc, True, fused)
        self._run_backward(None, None, None, backward_phase)
        return outs
