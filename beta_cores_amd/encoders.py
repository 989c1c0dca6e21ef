"""Device feature encoders: the learned map in front of the neural-linear model's regression head.

The neural-linear likelihood is the linear-regression formula on `[features(x), y]` (model_neurlinr.py), where `features` is a
small network -- Linear -> BatchNorm1d -> ReLU, twice (examples/common/neural.py).  `MLPEncoder` keeps such a network's
parameters on the device; `DeviceData.encode(enc)` turns resident raw rows into resident encoded rows (k_encode_mlp), and
`DeviceProjector(encoder=enc)` does so between the rows and K1, so a coreset holds, sub-samples and returns RAW rows.

A layer is `h <- act((W h + b) * scale + shift)`: W in torch's `Linear.weight` layout, an eval-mode batch norm folded into
`scale` and `shift`, `act` ReLU or the identity.  Everything is float64 on the device; float32 torch parameters are widened,
which is exact.  Training stays in torch: after it, hand the new parameters over with `update()` / `update_from_torch()`.
"""
import ctypes as C
import weakref

import numpy as np

from . import _native as N
from .device import _ptr, default_context, upload_slot

MAX_LAYERS = 4
MAX_WIDTH = 512


def _vec(v, n, what):
    if v is None:
        return None
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())
    if v.shape != (n,):
        raise ValueError('%s holds %d values, the layer has %d outputs' % (what, v.shape[0], n))
    return v


def _normalise(layers):
    """[(W, b, scale, shift, relu)] -> the same with float64 C-contiguous arrays (or None), widths checked."""
    layers = list(layers)
    if not 1 <= len(layers) <= MAX_LAYERS:
        raise ValueError('an encoder has 1..%d layers, got %d' % (MAX_LAYERS, len(layers)))
    out, widths = [], []
    for i, layer in enumerate(layers):
        W, b, s, t, relu = layer
        W = np.ascontiguousarray(np.asarray(W, dtype=np.float64))
        if W.ndim != 2:
            raise ValueError('layer %d: W must be 2-D (outputs x inputs)' % i)
        if widths and W.shape[1] != widths[-1]:
            raise ValueError('layer %d takes %d inputs, layer %d gives %d' % (i, W.shape[1], i - 1, widths[-1]))
        if not widths:
            widths.append(int(W.shape[1]))
        widths.append(int(W.shape[0]))
        n = W.shape[0]
        out.append((W, _vec(b, n, 'layer %d: b' % i), _vec(s, n, 'layer %d: scale' % i), _vec(t, n, 'layer %d: shift' % i), bool(relu)))
    for w in widths:
        if not 1 <= w <= MAX_WIDTH:
            raise ValueError('every width is in 1..%d, got %d' % (MAX_WIDTH, w))
    return out, tuple(widths)


def layers_from_torch(module):
    """An eval-mode `nn.Sequential` of Linear / BatchNorm1d / ReLU -> [(W, b, scale, shift, relu)] in float64.  A batch norm
    becomes scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale.  Needs no GPU."""
    import torch.nn as nn
    if not isinstance(module, nn.Sequential):
        raise ValueError('from_torch takes an nn.Sequential of Linear, BatchNorm1d and ReLU, got %s' % type(module).__name__)
    if module.training:
        raise ValueError('the module is in training mode: a batch norm then normalises by the batch, not by its running '
                         'statistics; call module.eval() first')
    f64 = lambda p: p.detach().cpu().numpy().astype(np.float64)
    layers = []      # [W, b, s, t, relu, has_bn]
    for i, m in enumerate(module):
        if isinstance(m, nn.Linear):
            layers.append([f64(m.weight), f64(m.bias) if m.bias is not None else None, None, None, False, False])
        elif isinstance(m, nn.BatchNorm1d):
            if not layers or layers[-1][4] or layers[-1][5]:
                raise ValueError('module %d: a BatchNorm1d must directly follow a Linear' % i)
            if m.training:
                raise ValueError('module %d: the BatchNorm1d is in training mode' % i)
            if m.running_mean is None or m.running_var is None:
                raise ValueError('module %d: a BatchNorm1d without running statistics has no eval-mode form' % i)
            n = layers[-1][0].shape[0]
            gamma = f64(m.weight) if m.weight is not None else np.ones(n)
            beta = f64(m.bias) if m.bias is not None else np.zeros(n)
            s = gamma / np.sqrt(f64(m.running_var) + float(m.eps))
            layers[-1][2] = s
            layers[-1][3] = beta - f64(m.running_mean) * s
            layers[-1][5] = True
        elif isinstance(m, nn.ReLU):
            if not layers or layers[-1][4]:
                raise ValueError('module %d: a ReLU must follow a Linear (or its BatchNorm1d)' % i)
            layers[-1][4] = True
        else:
            raise ValueError('module %d: %s is not supported (Linear, BatchNorm1d, ReLU)' % (i, type(m).__name__))
    if not layers:
        raise ValueError('the module has no Linear layer')
    return [tuple(l[:5]) for l in layers]


def _gamma(k, u):
    return k * u / (1. - k * u)


def host_forward(layers, x, dtype=np.float32, bound=False, u=2.0 ** -53):
    """The NumPy float64 restatement of the encoder on feature rows `x` (n x d[0]), its values rounded to `dtype` and held in
    float64.  `bound=True`: (float64 result BEFORE that rounding, e) with e an elementwise forward error bound for ANY
    evaluation of the same formula in arithmetic of unit roundoff `u`, in any summation order (gamma_k = k u / (1 - k u)):
        a = |W||h| + |b|;  e_pre = |W| e_in + 2 gamma_{K+2} a;  e_post = |s| e_pre + 4 u (|pre * s| + |t|)
    with e_in = 0 at the input; ReLU is 1-Lipschitz and leaves it unchanged.  (The factor 2 covers both sides: this
    restatement's own rounding and the other evaluation's.)  For tests and documentation; needs no GPU."""
    layers, widths = _normalise(layers)
    h = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if h.shape[1] != widths[0]:
        raise ValueError('rows have %d columns, the encoder takes %d' % (h.shape[1], widths[0]))
    e = np.zeros_like(h)
    for W, b, s, t, relu in layers:
        K = W.shape[1]
        bb = b if b is not None else np.zeros(W.shape[0])
        ss = s if s is not None else np.ones(W.shape[0])
        tt = t if t is not None else np.zeros(W.shape[0])
        pre = h.dot(W.T) + bb
        if bound:
            a = np.abs(h).dot(np.abs(W).T) + np.abs(bb)
            e = e.dot(np.abs(W).T) + 2. * _gamma(K + 2, u) * a
            e = np.abs(ss) * e + 4. * u * (np.abs(pre * ss) + np.abs(tt))
        h = pre * ss + tt
        if relu:
            h = np.where(h > 0, h, np.where(np.isnan(h), h, 0.))
    if bound:
        return h, e
    return h.astype(dtype).astype(np.float64)


class MLPEncoder:
    """A network of 1..4 layers `(W, b, scale, shift, relu)` resident on the device (see the module docstring).

    `.widths` -- (d[0], .., d[L]);  `.version` -- bumped by every update(), what caches of encoded rows are keyed by.
    `enc(pts)` encodes a few host rows ON THE DEVICE (the <= M coreset points a sampler sees get the very bits the data rows
    get); `DeviceData.encode(enc)` is the bulk path; `host()` is the NumPy restatement for tests."""

    def __init__(self, layers, ctx=None):
        self.layers, self.widths = _normalise(layers)
        self.ctx = ctx or default_context()
        w = np.ascontiguousarray(self.widths, dtype=np.int32)
        h = C.c_void_p()
        N.call('bc_encoder_create', self.ctx.h, len(self.layers), _ptr(w), C.byref(h))
        self.h = h
        self._fin = weakref.finalize(self, N.load().bc_encoder_destroy, h)
        self.version = 0
        self.launches = 0          # bc_data_encode calls made with this encoder
        self._slots = {}           # input columns -> upload slot of __call__
        self._outs = {}            # (pass_cols, dtype) -> re-used output buffer of __call__
        self._upload()

    def _upload(self):
        for l, (W, b, s, t, relu) in enumerate(self.layers):
            N.call('bc_encoder_set_layer', self.h, l, _ptr(W), _ptr(b), _ptr(s), _ptr(t), 1 if relu else 0)

    @classmethod
    def from_torch(cls, module, ctx=None):
        return cls(layers_from_torch(module), ctx=ctx)

    def update(self, layers):
        """New parameters for the same widths (after the network was retrained): re-uploads, bumps `.version`."""
        layers, widths = _normalise(layers)
        if widths != self.widths:
            raise ValueError('update() keeps the widths %s, got %s' % (self.widths, widths))
        self.layers = layers
        self._upload()
        self.version += 1
        return self

    def update_from_torch(self, module):
        return self.update(layers_from_torch(module))

    def out_width(self, pass_cols=0):
        return self.widths[-1] + int(pass_cols)

    def host(self, x, dtype=np.float32, bound=False, u=2.0 ** -53):
        return host_forward(self.layers, x, dtype=dtype, bound=bound, u=u)

    def __call__(self, pts, pass_cols=1, dtype=np.float32):
        """Host rows `[x, pass-through]` -> host rows `[features, pass-through]` (float64 holding `dtype`'s values), computed
        on the device through an upload slot.  For the few coreset points; bulk rows go through DeviceData.encode."""
        pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
        if pts.size == 0:
            return np.zeros((0, self.out_width(pass_cols)))
        if pts.shape[1] != self.widths[0] + pass_cols:
            raise ValueError('rows have %d columns, the encoder takes %d + %d pass-through' % (pts.shape[1], self.widths[0], pass_cols))
        slot = upload_slot(self._slots, pts.shape[1], self.ctx)
        key = (int(pass_cols), np.dtype(dtype).str)
        out = self._outs[key] = slot.update(pts).encode(self, pass_cols=pass_cols, dtype=dtype, out=self._outs.get(key))
        return out.rows(np.arange(pts.shape[0]))
