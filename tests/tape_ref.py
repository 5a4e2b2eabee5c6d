"""NumPy float64 reference of every fp32 tape op of csrc/bwd.hip, pool.hip, glue.hip, crf.hip, finetune.hip and of soft_hist_bwd /
lin_frontend_bwd (csrc/frontend.hip, finetune.hip), written from the op's definition -- test infrastructure.

The definitions that do not depend on the storage format (pools, resize, upsample, gap, BatchNorm, act_grad, add, pack / unpack,
the front end) are the ones of tests/fp16_ref.py, imported below and re-exported under the same names; this module adds the ops
that only the fp32 tape has.  Nothing here calls the package under test.  Where oracle/ops.py states an op it is reused; the
backward ops are pinned against float64 autograd (tests/torch_ref.py) by tests/test_tape_ref.py.  Every function takes and returns
float64 arrays; the fp32 roundings of the kernels are NOT applied -- the GPU tests put them into their bars (`bar32`, `sum_bar`) or
make them vanish by choosing inputs whose results are exactly representable.
"""
import numpy as np

from fp16_ref import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, U32, _f, abs_bound, act_bwd_bias, act_grad, add, avgpool2,  # noqa: F401
                      avgpool2_bwd, bn_apply, bn_bwd, bn_stats, gap, gap_bwd, lin_frontend, lin_frontend_abs, lin_frontend_bwd,
                      maxpool2, maxpool2_bwd, maxpool3s2, maxpool3s2_bwd, pack3, pad_channels, resize2x, resize2x_bwd, ulp32,
                      unpack3, upsample_zero2)
from oracle import ops

NPCA = 11


# ---- bars ------------------------------------------------------------------------------------------------------------------------
def bar32(k, B):
    """k fp32 roundings (round to nearest, unit round-off 2^-24) on a path whose magnitudes B bounds"""
    return k * U32 * np.abs(_f(B))


def sum_bar(terms, axis=None, extra=0):
    """the standard bound of an fp32 sum of n terms in ANY order and grouping: (n - 1) 2^-24 sum |terms| (first order; the factor
    (1 + 2^-24)^(n-1) is absorbed by `extra` roundings of the terms themselves, which the caller counts)"""
    t = np.abs(_f(terms))
    n = t.size if axis is None else t.shape[axis]
    return (n - 1 + extra) * U32 * t.sum(axis=axis)


# ---- elementwise glue --------------------------------------------------------------------------------------------------------------
def clip(x, lo, hi):
    return np.minimum(np.maximum(_f(x), lo), hi)


def clip_bwd(dy, x, lo, hi):
    """tf.clip_by_value: the gradient passes on the CLOSED interval [lo, hi]"""
    x = _f(x)
    return np.where((x >= lo) & (x <= hi), _f(dy), 0.0)


def logc(x):
    return ops.log_compress(_f(x))


def logc_bwd(dy, x):
    return _f(dy) * 10.0 / ((1.0 + 10.0 * _f(x)) * np.log(11.0))


def reverse3(x):
    return _f(x)[..., ::-1].copy()


def vgg_preprocess(x, out_channels=3):
    return pad_channels(ops.vgg_preprocess(_f(x)), out_channels)


def vgg_preprocess_bwd(dy):
    """d rgb = 255 * reverse3(d bgr[:3]); a fourth (padding) channel carries no gradient"""
    return _f(dy)[..., 2::-1] * 255.0


def alpha_mask(x, thr=0.12):
    """[..., 1]: clamp((max_c x - 1 + thr) / thr, 0, 1)"""
    return ops.alpha_mask(_f(x), thr)[..., :1]


def alpha_blend(b, hal, thr=0.12):
    """(A, alpha) of A = B + alpha(B) * reverse3(hal)"""
    b = _f(b)
    al = alpha_mask(b, thr)
    return b + al * reverse3(hal), al


def alpha_blend_bwd(dA, alpha):
    """alpha a constant: d hal = reverse3(alpha * dA)"""
    return reverse3(_f(alpha) * _f(dA))


def alpha_blend_full_bwd(b, hal, dA, thr):
    """(dB, dhal) with the gradient through alpha(B): it reaches the FIRST maximal channel of B where 0 < alpha < 1"""
    b, dA = _f(b), _f(dA)
    hr = reverse3(hal)
    u = b.max(axis=-1, keepdims=True) - 1.0 + thr
    al = np.minimum(1.0, np.maximum(0.0, u) / thr)
    live = (u > 0.0) & (u / thr < 1.0)
    dal = np.where(live, (dA * hr).sum(axis=-1, keepdims=True) / thr, 0.0)
    hot = np.arange(3) == b.argmax(axis=-1)[..., None]
    return dA + hot * dal, reverse3(al * dA)


def act(v, a):
    v = _f(v)
    if a == ACT_RELU:
        return np.maximum(v, 0.0)
    if a == ACT_LRELU:
        return np.where(v >= 0.0, v, 0.1 * v)
    if a == ACT_TANH:
        return np.tanh(v)
    return v


def affine_pre(x, scale=None, shift=None, residual=None, absolute=False):
    """x * scale[c] + shift[c] + residual, each optional; absolute: the same over magnitudes (bounds every partial sum)"""
    ab = np.abs if absolute else (lambda t: t)
    v = ab(_f(x))
    if scale is not None:
        v = v * ab(_f(scale))
    if shift is not None:
        v = v + ab(_f(shift))
    if residual is not None:
        v = v + ab(_f(residual))
    return v


def affine_act(x, scale=None, shift=None, residual=None, a=ACT_NONE):
    return act(affine_pre(x, scale, shift, residual), a)


# ---- inverse-CRF head ----------------------------------------------------------------------------------------------------------------
def invcrf_decode(feat, wfc, bfc, table):
    """Dense(11) + PCA decode: table[:, 0] + table[:, 1:12] @ (feat @ wfc + bfc)"""
    table = _f(table)
    return ops.invcrf_pca_decode(ops.dense(_f(feat), _f(wfc), _f(bfc)), table[:, 0], table[:, 1:1 + NPCA])


def invcrf_decode_bwd(dinv, feat, wfc, table, absolute=False):
    """(dfeat, dwfc, dbfc); dwfc and dbfc summed over the batch"""
    ab = np.abs if absolute else (lambda t: t)
    dw = ab(_f(dinv)) @ ab(_f(table)[:, 1:1 + NPCA])                 # [B, 11]
    return dw @ ab(_f(wfc)).T, ab(_f(feat)).T @ dw, dw.sum(axis=0)


def increase(rf):
    return ops.increase(_f(rf))


def increase_bwd(rf, dout):
    """backward of `_increase`; the gradient of the row minimum goes to its FIRST occurrence (TF spreads it over ties: inputs with a
    tied minimum are outside this reference)"""
    rf, dout = _f(rf), _f(dout)
    g = rf[:, 1:] - rf[:, :-1]
    mn, arg = g.min(axis=1), g.argmin(axis=1)
    ng = g + np.maximum(-mn, 0.0)[:, None]
    S = ng.sum(axis=1, keepdims=True)
    dn = np.cumsum(dout[:, :0:-1], axis=1)[:, ::-1]                 # d loss / d (ng / S)[k] = sum_{j >= k} dout[j + 1]
    d = dn / S - (dn * ng).sum(axis=1, keepdims=True) / (S * S)
    rows = np.arange(rf.shape[0])
    d[rows, arg] -= np.where(mn < 0.0, d.sum(axis=1), 0.0)
    drf = np.zeros_like(rf)
    drf[:, 1:] += d
    drf[:, :-1] -= d
    return drf


def apply_rf(x, rf):
    return ops.apply_rf(_f(x), _f(rf))


def apply_rf_parts(x, K):
    """(yv, i0, i1, w0, w1) of the K-entry look-up: y = w0 rf[i0] + w1 rf[i1]"""
    x = _f(x)
    b = x.shape[0]
    yv = (K - 1.0) * x.reshape(b, -1)
    y0 = np.floor(yv)
    i0 = np.clip(y0.astype(np.int64), 0, K - 1)
    i1 = np.clip(y0.astype(np.int64) + 1, 0, K - 1)
    return yv, i0, i1, (y0 + 1.0) - yv, yv - y0


def apply_rf_bwd(x, rf, dy, absolute=False):
    """(drf, dx): drf[b, i0] += dy w0, drf[b, i1] += dy w1; dx = dy (K - 1) (rf[i1] - rf[i0])"""
    rf = _f(rf)
    b, K = rf.shape
    _, i0, i1, w0, w1 = apply_rf_parts(x, K)
    g = _f(dy).reshape(b, -1)
    if absolute:
        g, w0, w1 = np.abs(g), np.abs(w0), np.abs(w1)
    drf = np.zeros_like(rf)
    rows = np.broadcast_to(np.arange(b)[:, None], i0.shape)
    np.add.at(drf, (rows, i0), g * w0)
    np.add.at(drf, (rows, i1), g * w1)
    l0, l1 = np.take_along_axis(rf, i0, 1), np.take_along_axis(rf, i1, 1)
    dx = g * (K - 1.0) * ((np.abs(l1) + np.abs(l0)) if absolute else (l1 - l0))
    return drf, dx.reshape(np.shape(x))


# ---- losses --------------------------------------------------------------------------------------------------------------------------
def diff_loss(a, b, mode):
    """[B]: per-sample mean of (a - b)^2 (mode 0) or |a - b| (mode 1) -- the sum divided ONCE by the element count"""
    d = (_f(a) - _f(b)).reshape(np.shape(a)[0], -1)
    return (np.abs(d) if mode else d * d).sum(axis=1) / d.shape[1]


def diff_loss_bwd(a, b, g, mode, da0=None):
    """g[b] / n * (2 (a - b) | sign(a - b)); da0: the destination's content when the kernel accumulates"""
    a = _f(a)
    d = a - _f(b)
    n = d.size // d.shape[0]
    gb = (_f(g) / n).reshape((-1,) + (1,) * (d.ndim - 1))
    v = gb * (np.sign(d) if mode else 2.0 * d)
    return v if da0 is None else _f(da0) + v


def tv_terms(y):
    """(vertical, horizontal) forward differences of NHWC y"""
    y = _f(y)
    return y[:, 1:] - y[:, :-1], y[:, :, 1:] - y[:, :, :-1]


def tv_loss(y):
    """(sum |dv| + sum |dh|) / (N H W C): the two means of joint_training.py:175-179 share their denominator"""
    dv, dh = tv_terms(y)
    return (np.abs(dv).sum() + np.abs(dh).sum()) / np.size(y)


def tv_sign_sum(y):
    """d (sum |dv| + sum |dh|) / dy: an integer in [-4, 4] per element"""
    dv, dh = tv_terms(y)
    s = np.zeros(np.shape(y))
    s[:, :-1] -= np.sign(dv)
    s[:, 1:] += np.sign(dv)
    s[:, :, :-1] -= np.sign(dh)
    s[:, :, 1:] += np.sign(dh)
    return s


def tv_loss_bwd(y, g, dy0=None):
    v = float(np.asarray(g).reshape(-1)[0]) / np.size(y) * tv_sign_sum(y)
    return v if dy0 is None else _f(dy0) + v


def sample_dot(a, b=None):
    a = _f(a).reshape(np.shape(a)[0], -1)
    return (a if b is None else a * _f(b).reshape(a.shape)).sum(axis=1)


def _per(v, ndim):
    return _f(v).reshape((-1,) + (1,) * (ndim - 1))


def mean_norm_fwd(r, ssum, eps, target):
    """r / (eps + ssum / n) * target, ssum the per-sample sum of r"""
    r = _f(r)
    n = r.size // r.shape[0]
    return r / (eps + _per(ssum, r.ndim) / n) * target


def mean_norm_bwd(g, ssum, gdot, eps, target, absolute=False):
    """target (g / d - gdot / (n d^2)), d = eps + ssum / n, gdot = <g, r> per sample"""
    g = _f(g)
    n = g.size // g.shape[0]
    d = eps + _per(ssum, g.ndim) / n
    if absolute:
        return np.abs(target) * (np.abs(g) / np.abs(d) + np.abs(_per(gdot, g.ndim)) / (n * d * d))
    return target * (g / d - _per(gdot, g.ndim) / (n * d * d))


# ---- soft histogram ----------------------------------------------------------------------------------------------------------------
def soft_hist(img, B):
    return ops.histogram_layer(_f(img), B)


def soft_hist_bwd(img, dy, B, absolute=False):
    """dx[.., c] = sum over bins i of dy[.., (i - 1) C + c] * (-B sign(x - centre_i)) inside the support |x - centre_i| < 1 / B"""
    img, dy = _f(img), _f(dy)
    c = img.shape[-1]
    dx = np.zeros_like(img)
    for i in range(1, B + 1):
        d = img - (2.0 * i - 1.0) / (2.0 * B)
        slope = np.where(np.abs(d) < 1.0 / B, -B * np.sign(d), 0.0)
        g = dy[..., (i - 1) * c:i * c]
        dx += np.abs(g * slope) if absolute else g * slope
    return dx


# ---- Keras Adam ----------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, lr_t, b1, b2, eps, grad_scale=1.0):
    """(p, m, v) after one step: g' = g * grad_scale; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2;
    p -= lr_t m / (sqrt(v) + eps)   (Keras: eps outside the root, the bias correction folded into lr_t)"""
    p, g, m, v = _f(p), _f(g) * grad_scale, _f(m), _f(v)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v
