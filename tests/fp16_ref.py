"""NumPy float64 reference of every fp16 tape op of csrc/elem_f16.hip, written from the op's definition -- test infrastructure.

Nothing here calls the package under test.  Where oracle/ops.py already states an op it is reused; the backward ops are written out
here and pinned against float64 autograd (tests/torch_ref.py) by tests/test_fp16_ref.py.  Every function takes and returns float64
NHWC arrays (it widens whatever it is given); the rounding of the stored fp16 result is NOT applied -- the GPU tests put it into
their bar through `ulp16`, or make it vanish by choosing inputs whose results are exactly representable.
"""
import numpy as np

from oracle import ops

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
U32 = 2.0 ** -24          # unit round-off of one fp32 operation (round to nearest)


def _f(x):
    return np.asarray(x, dtype=np.float64)


def ulp16(v):
    """spacing of the fp16 grid at |v|: 2^(e - 10) for 2^e <= |v| < 2^(e+1), the subnormal spacing 2^-24 below 2^-14"""
    a = np.abs(_f(v))
    _, ex = np.frexp(a)                                  # |v| = m * 2^ex, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(np.where(a > 0, ex - 1, -14), -14) - 10)


def ulp32(v):
    a = np.abs(_f(v))
    _, ex = np.frexp(a)
    return np.ldexp(1.0, np.maximum(np.where(a > 0, ex - 1, -126), -126) - 23)


# ---- casts / packing -------------------------------------------------------------------------------------------------------
def cast_f16(x):
    """IEEE round-to-nearest-even conversion (NumPy's), as a float16 array"""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16)


def pad_channels(x, channels):
    x = np.asarray(x)
    y = np.zeros(x.shape[:-1] + (channels,), dtype=x.dtype)
    y[..., :x.shape[-1]] = x
    return y


def pack3(srcs, out_channels, vgg=False):
    """concat of 3-channel images, zero-padded to out_channels; vgg: oracle.ops.vgg_preprocess of the single source"""
    srcs = [_f(s) for s in srcs]
    cat = ops.vgg_preprocess(srcs[0]) if vgg else np.concatenate(srcs, axis=-1)
    return pad_channels(cat, out_channels)


def pack3_vgg_abs(src):
    """magnitudes on the path of x * 255 - mean"""
    return np.abs(_f(src))[..., ::-1] * 255.0 + np.asarray(ops.VGG_MEAN)


def unpack3(y, nout, vgg=False):
    """the first nout 3-channel slices; vgg: the backward of the preprocessing (d/dx of x*255, RGB->BGR, minus mean)"""
    y = _f(y)
    if vgg:
        return (y[..., 2::-1] * 255.0,)
    return tuple(y[..., 3 * s:3 * s + 3] for s in range(nout))


# ---- activation backward + bias gradient -----------------------------------------------------------------------------------
def act_grad(dy, y, act):
    dy = _f(dy)
    if act == ACT_NONE:
        return dy
    y = _f(y)
    if act == ACT_RELU:
        return np.where(y > 0, dy, 0.0)
    if act == ACT_LRELU:
        return np.where(y > 0, dy, 0.1 * dy)
    return dy * (1.0 - y * y)


def act_bwd_bias(dy, y, act):
    dz = act_grad(dy, y, act)
    return dz, dz.reshape(-1, dz.shape[-1]).sum(axis=0)


def add(a, b, relu=False):
    s = _f(a) + _f(b)
    return np.maximum(s, 0.0) if relu else s


# ---- pooling / resize --------------------------------------------------------------------------------------------------------
def avgpool2(x):
    return ops.avg_pool2(_f(x))


def avgpool2_bwd(dy, x_shape):
    """every cell of a complete 2x2 window gets dy / 4; the last row / column of an odd size belongs to no window: zero"""
    n, h, w, c = x_shape
    dy = _f(dy)
    dx = np.zeros(x_shape)
    ho, wo = h // 2, w // 2
    dx[:, :2 * ho, :2 * wo] = np.repeat(np.repeat(dy, 2, axis=1), 2, axis=2) * 0.25
    return dx


def maxpool2(x):
    return ops.max_pool(_f(x), 2, 2)


def maxpool2_bwd(x, dy):
    """the gradient goes to the FIRST maximum of the window in row-major order (np.argmax returns the first)"""
    x, dy = _f(x), _f(dy)
    n, h, w, c = x.shape
    win = x.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    hot = np.arange(4) == win.argmax(axis=-1)[..., None]
    dx = hot * dy[..., None]
    return dx.reshape(n, h // 2, w // 2, c, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, h, w, c)


def maxpool3s2(x):
    return ops.max_pool(_f(x), 3, 2)


def maxpool3s2_bwd(x, dy):
    """MaxPool2D(3, 2, SAME): every window hands its gradient to its first maximum in row-major order; padded cells never win;
    the windows overlap, so an element may collect several"""
    x, dy = _f(x), _f(dy)
    n, h, w, c = x.shape
    ho, pt, pb = ops.same_pad(h, 3, 2)
    wo, pl, pr = ops.same_pad(w, 3, 2)
    xp = np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)), constant_values=-np.inf)
    taps = [(i, j) for i in range(3) for j in range(3)]
    sl = lambda i, j: (slice(None), slice(i, i + 2 * (ho - 1) + 1, 2), slice(j, j + 2 * (wo - 1) + 1, 2))
    best = np.full(dy.shape, -np.inf)
    arg = np.zeros(dy.shape, dtype=np.int64)
    for t, (i, j) in enumerate(taps):
        v = xp[sl(i, j)]
        better = v > best
        best = np.where(better, v, best)
        arg = np.where(better, t, arg)
    dxp = np.zeros(xp.shape)
    for t, (i, j) in enumerate(taps):
        dxp[sl(i, j)] += np.where(arg == t, dy, 0.0)
    return dxp[:, pt:pt + h, pl:pl + w]


def _resize_matrix(n_in):
    """[2 n_in, n_in] weights of tf.image.resize(2x, BILINEAR), half-pixel centres, clamped taps"""
    m = np.zeros((2 * n_in, n_in))
    for d in range(2 * n_in):
        src = (d + 0.5) * 0.5 - 0.5
        f = np.floor(src)
        lo, hi, t = int(max(f, 0)), int(min(np.ceil(src), n_in - 1)), src - f
        m[d, lo] += 1.0 - t
        m[d, hi] += t
    return m


def resize2x(x):
    return ops.resize_bilinear_2x(_f(x))


def resize2x_bwd(dy, x_shape):
    """the transpose of the (linear) forward"""
    n, h, w, c = x_shape
    t = np.tensordot(_resize_matrix(h).T, _f(dy), axes=([1], [1]))            # [h, n, 2w, c]
    t = np.tensordot(_resize_matrix(w).T, t, axes=([1], [2]))                 # [w, h, n, c]
    return np.ascontiguousarray(t.transpose(2, 1, 0, 3))


def upsample_zero2(dy, x_shape):
    """the input gradient of a stride-2 subsampling: dy at the even positions, zero elsewhere"""
    dx = np.zeros(x_shape)
    dx[:, ::2, ::2] = _f(dy)
    return dx


def gap(x):
    return ops.global_avg_pool(_f(x))


def gap_bwd(dy, x_shape):
    n, h, w, c = x_shape
    return np.broadcast_to(_f(dy)[:, None, None, :] / (h * w), x_shape).copy()


# ---- training-mode BatchNorm -------------------------------------------------------------------------------------------------
def bn_stats(x):
    """batch mean and BIASED variance over (N, H, W)"""
    _, mean, var = ops.batch_norm_train(_f(x), np.ones(x.shape[-1]), np.zeros(x.shape[-1]))
    return mean, var


def bn_apply(x, mean, var, gamma, beta, eps, relu):
    y = (_f(x) - _f(mean)) / np.sqrt(_f(var) + eps) * _f(gamma) + _f(beta)
    return np.maximum(y, 0.0) if relu else y


def bn_bwd(dy, x, y_relu, mean, var, gamma, eps, absolute=False):
    """(dx, dgamma, dbeta) of y = [relu](gamma * (x - mean) / sqrt(var + eps) + beta) with mean / var the batch statistics of x;
    the relu mask is y_relu > 0.  absolute=True: the same expressions over magnitudes (the bound B of the GPU tests)"""
    g, x = _f(dy), _f(x)
    if y_relu is not None:
        g = np.where(_f(y_relu) > 0, g, 0.0)
    rstd = 1.0 / np.sqrt(_f(var) + eps)
    xc = x - _f(mean)
    if absolute:
        g, xc, gamma = np.abs(g), np.abs(x) + np.abs(_f(mean)), np.abs(_f(gamma))
    xh = xc * rstd
    dbeta = g.reshape(-1, g.shape[-1]).sum(axis=0)
    dgamma = (g * xh).reshape(-1, g.shape[-1]).sum(axis=0)
    npix = g.size // g.shape[-1]
    sign = 1.0 if absolute else -1.0
    dx = _f(gamma) * rstd * (g + sign * dbeta / npix + sign * xh * dgamma / npix)
    return dx, dgamma, dbeta


# ---- Linearization-Net front end -----------------------------------------------------------------------------------------------
def lin_frontend(img, channels=96):
    """[img 3 | sobel 6 | hist4 12 | hist8 24 | hist16 48 | zeros]"""
    return pad_channels(ops.lin_frontend(_f(img)), channels)


def lin_frontend_abs(img, channels=96):
    """per-channel bound of the magnitudes on the front end's paths: |img|, sum |k| |img| for the sobel channels, 1 + |d| B <= 2 for
    the histogram channels"""
    a = np.abs(_f(img))
    n, h, w, c = a.shape
    xp = np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="reflect")
    ky = np.abs(np.array([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], dtype=np.float64))
    sy = sum(ky[i, j] * xp[:, i:i + h, j:j + w] for i in range(3) for j in range(3))
    sx = sum(ky.T[i, j] * xp[:, i:i + h, j:j + w] for i in range(3) for j in range(3))
    sob = np.stack([sy, sx], axis=-1).reshape(n, h, w, 2 * c)
    return pad_channels(np.concatenate([a, sob, np.full((n, h, w, 84), 2.0)], axis=-1), channels)


def lin_frontend_bwd(img, dF, absolute=False):
    """dimg = dF[image] + sobel^T dF[sobel] + sum over bins of dF[hist] * d/dx (1 - |x - centre| B) inside the support;
    absolute=True: the same sums over magnitudes"""
    img, dF = _f(img), _f(dF)
    if absolute:
        dF = np.abs(dF)
    n, h, w, c = img.shape
    dimg = dF[..., :3].copy()
    ky = np.array([[-1, -2, -1], [0, 0, 0], [1, 2, 1]], dtype=np.float64)
    refl = lambda i, m: np.where(i < 0, -i, np.where(i >= m, 2 * m - 2 - i, i))
    for i in range(3):
        rh = refl(np.arange(h) + i - 1, h)
        for j in range(3):
            rw = refl(np.arange(w) + j - 1, w)
            for k, kern in enumerate((ky, ky.T)):
                wt = abs(kern[i, j]) if absolute else kern[i, j]
                if wt != 0:
                    np.add.at(dimg, (slice(None), rh[:, None], rw[None, :]), wt * dF[..., 3 + k:9:2])
    for B, off in ((4, 9), (8, 21), (16, 45)):
        for b in range(1, B + 1):
            d = img - (2.0 * b - 1.0) / (2.0 * B)
            slope = np.where(np.abs(d) < 1.0 / B, -B * np.sign(d), 0.0)
            dimg += dF[..., off + 3 * (b - 1):off + 3 * b] * (np.abs(slope) if absolute else slope)
    return dimg


# ---- bounds --------------------------------------------------------------------------------------------------------------------
_LINEAR = {"avgpool2": avgpool2, "avgpool2_bwd": avgpool2_bwd, "resize2x": resize2x, "resize2x_bwd": resize2x_bwd,
           "add": add, "gap": gap, "gap_bwd": gap_bwd, "upsample_zero2": upsample_zero2}


def abs_bound(op, x, *args):
    """for an op that is linear with fixed non-negative weights: the same op applied to |x| -- it bounds every partial sum on the
    path to an output element (`add`: abs_bound("add", a, b))"""
    return _LINEAR[op](np.abs(_f(x)), *[np.abs(_f(a)) if isinstance(a, np.ndarray) else a for a in args])
