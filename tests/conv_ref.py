"""float64 NumPy statement of the three convolution operations of the native-fp16 path, with the conventions of `shdr_conv2d_desc`
(include/shdr.h): NHWC tensors, HWIO filters, cross-correlation, TF 'SAME' padding (the extra cell goes to the bottom / right, so a
stride-2 layer is padded asymmetrically), two sources concatenated along the channels with the second one scaled by `x2_scale`.

It calls nothing of the product.  tests/test_conv_ref.py pins it to oracle.ops.conv2d and to float64 autograd;
tests/test_gpu_fp16_conv_exact.py compares the HIP kernels with it element by element,
tests/test_gpu_wgrad_f32_exact.py the fp32 weight-gradient kernels (section 4.4), tests/test_gpu_conv_x3_exact.py the split-operand
kernels (section 4.5), tests/test_gpu_up2_lowres_exact.py the low-resolution channel mix (section 4.6) and tests/test_gpu_conv_f32_exact.py the
exact-fp32 kernels: implicit GEMM, register-A, direct, Winograd, the input-gradient plumbing (section 4.7).
"""
import numpy as np

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
LRELU_SLOPE = np.float32(0.1)              # the fp32 constant of the kernels (shdr::act_apply: v * 0.1f)


def same_pad(size, k, stride):
    """(output size, padding before) of TF 'SAME'"""
    out = -(-size // stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def _geometry(h, w, kh, kw, stride, pad, out_hw):
    ho, pt = same_pad(h, kh, stride)
    wo, pl = same_pad(w, kw, stride)
    if pad is not None:
        pt, pl = pad
    if out_hw is not None:
        ho, wo = out_hw
    return ho, wo, pt, pl


def _padded(x, kh, kw, stride, ho, wo, pt, pl):
    """x zero-padded so that output (oh, ow) and tap (a, b) read xp[:, oh * stride + a, ow * stride + b]"""
    n, h, w, c = x.shape
    pb = max((ho - 1) * stride + kh - pt - h, 0)
    pr = max((wo - 1) * stride + kw - pl - w, 0)
    return np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))


def _sources(x, x2, x2_scale):
    x = np.asarray(x, dtype=np.float64)
    if x2 is None:
        return x
    return np.concatenate([x, np.asarray(x2, dtype=np.float64) * float(x2_scale)], axis=-1)


def conv2d(x, x2, w, bias, stride, x2_scale, pad=None, out_hw=None):
    """z[n, oh, ow, co] = bias[co] + sum_{a, b, c} xin[n, oh * stride - pad_t + a, ow * stride - pad_l + b, c] * w[a, b, c, co],
    xin = concat[x, x2_scale * x2]; cells outside the input are zero.  `pad` = (pad_t, pad_l) and `out_hw` = (Ho, Wo) replace the
    'SAME' values, as `_ops.conv2d_h` takes them (the polyphase input gradient)."""
    xin = _sources(x, x2, x2_scale)
    w = np.asarray(w, dtype=np.float64)
    n, h, wd, c = xin.shape
    kh, kw, cin, cout = w.shape
    assert cin == c, (xin.shape, w.shape)
    ho, wo, pt, pl = _geometry(h, wd, kh, kw, stride, pad, out_hw)
    xp = _padded(xin, kh, kw, stride, ho, wo, pt, pl)
    z = np.zeros((n, ho, wo, cout))
    for a in range(kh):
        for b in range(kw):
            z += xp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride] @ w[a, b]
    if bias is not None:
        z += np.asarray(bias, dtype=np.float64)[:cout]
    return z


def dgrad(dz, w, x_shape, c_begin, c_count, scale, stride):
    """gradient of sum(z * dz) w.r.t. ONE source of the 'SAME' forward conv: the source owns filter rows [c_begin, c_begin + c_count)
    and enters the conv multiplied by `scale`.  dz may carry more channels per pixel than the filter has columns (a zero-padded head):
    the extra ones carry no gradient."""
    dz = np.asarray(dz, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    n, h, wd, c = x_shape
    assert c == c_count
    kh, kw, _, cout = w.shape
    ho, wo, pt, pl = _geometry(h, wd, kh, kw, stride, None, None)
    assert dz.shape[:3] == (n, ho, wo) and dz.shape[3] >= cout, (dz.shape, (n, ho, wo, cout))
    dz = dz[..., :cout]
    dxp = np.zeros_like(_padded(np.zeros((n, h, wd, c)), kh, kw, stride, ho, wo, pt, pl))
    for a in range(kh):
        for b in range(kw):
            dxp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride] += dz @ w[a, b, c_begin:c_begin + c_count].T
    return float(scale) * dxp[:, pt:pt + h, pl:pl + wd]


def wgrad(x, x2, dz, w_shape, stride, x2_scale, cout_valid):
    """gradient of sum(z * dz) w.r.t. the filter [kh, kw, C1 + C2, Cout]: rows [0, C1) from x, rows [C1, C1 + C2) from x2 (times
    x2_scale); columns >= cout_valid are zero (dz channels beyond them are ignored)."""
    dz = np.asarray(dz, dtype=np.float64)
    kh, kw, cin, cout = w_shape
    dw = np.zeros((kh, kw, cin, cout))
    cv = cout if cout_valid is None else cout_valid
    row = 0
    for src, s in ((x, 1.0), (x2, float(x2_scale))):
        if src is None:
            continue
        src = np.asarray(src, dtype=np.float64)
        n, h, wd, c = src.shape
        ho, wo, pt, pl = _geometry(h, wd, kh, kw, stride, None, None)
        assert dz.shape[:3] == (n, ho, wo), (dz.shape, (n, ho, wo))
        xp = _padded(src, kh, kw, stride, ho, wo, pt, pl)
        for a in range(kh):
            for b in range(kw):
                patch = xp[:, a:a + (ho - 1) * stride + 1:stride, b:b + (wo - 1) * stride + 1:stride]
                dw[a, b, row:row + c, :cv] = s * np.tensordot(patch, dz[..., :cv], axes=([0, 1, 2], [0, 1, 2]))
        row += c
    assert row == cin, (row, cin)
    return dw


def _act32(v, act):
    if act == ACT_RELU:
        return np.maximum(v, np.float32(0.0))
    if act == ACT_LRELU:
        return np.where(v >= 0, v, v * LRELU_SLOPE).astype(np.float32)          # ONE fp32 product with the kernel's constant
    if act == ACT_TANH:
        return np.tanh(v.astype(np.float64)).astype(np.float32)                  # (the one step that is not exact: see the GPU test)
    return v


def epilogue(z, act1, scale=None, shift=None, residual=None, act2=ACT_NONE):
    """the inference epilogue of shdr_conv2d_fwd_fused_f16 after the fp32 accumulator + bias `z`, in the kernel's order
    (shdr::fused_epi4_f16): act1, * scale[co], + shift[co], + residual, act2.  Every step is fp32 and rounded once; the result is the fp32
    value that is stored (fp32 heads) or cast to fp16 (`to_f16`).  With scale a power of two the product is exact, so a compiler that
    contracts `v * scale + shift` into one FMA computes the same value."""
    v = np.asarray(z, dtype=np.float64).astype(np.float32)
    c = v.shape[-1]
    v = _act32(v, act1)
    if scale is not None:
        v = (v * np.asarray(scale, dtype=np.float32)[:c]).astype(np.float32)
    if shift is not None:
        v = (v + np.asarray(shift, dtype=np.float32)[:c]).astype(np.float32)
    if residual is not None:
        v = (v + np.asarray(residual)[..., :c].astype(np.float32)).astype(np.float32)
    return _act32(v, act2)


def to_f16(v):
    """round to nearest even, ONE rounding from the float64 value (2049 -> 2048, 2051 -> 2052)"""
    return np.asarray(v, dtype=np.float64).astype(np.float16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp32 weight-gradient helpers (csrc/wgrad.hip, wgrad_x3.hip), for tests/test_gpu_wgrad_f32_exact.py
# ---------------------------------------------------------------------------------------------------------------------------------
def bias_grad(dz):
    """db[c] = sum over every pixel of dz[..., c]"""
    dz = np.asarray(dz, dtype=np.float64)
    return dz.reshape(-1, dz.shape[-1]).sum(axis=0)


def filter_transform(w, c_begin, c_count, scale):
    """wt[kh, kw, co, ci - c_begin] = scale * w[KH - 1 - kh, KW - 1 - kw, ci, co], ci in [c_begin, c_begin + c_count): the filter of the
    input gradient written as a forward convolution on dz (include/shdr.h: shdr_filter_transform_f32)"""
    w = np.asarray(w, dtype=np.float64)
    assert 0 <= c_begin and 0 < c_count and c_begin + c_count <= w.shape[2]
    return float(scale) * np.ascontiguousarray(w[::-1, ::-1, c_begin:c_begin + c_count, :].transpose(0, 1, 3, 2))


def range_exponent(bound):
    """T = 11 - (frexp exponent of the fp32 bound in a range slot): 2^T brings the bound to [2^10, 2^11).  0 for a slot that holds no
    bound -- zero, infinity, a NaN pattern, or a word with the sign bit set (the kernel compares the slot's bits as an unsigned
    number); clamped to +-126.  (No finite fp32 bound reaches the lower clamp: the largest one gives T = -117.)"""
    b = int(np.asarray(bound, dtype=np.float32).view(np.uint32))
    if b == 0 or b >= 0x7F800000:
        return 0
    _, ex = np.frexp(np.float64(np.float32(bound)))
    return int(min(max(11 - int(ex), -126), 126))


def split_planes(x, bound):
    """(hi, lo) fp16 planes of an fp32 tensor as shdr::split4 (csrc/split.h) states them: hi = fp16(x 2^T), lo = fp16(fp32(x 2^T - hi) 2^11),
    T = range_exponent(bound), every conversion round-to-nearest-even.  x 2^T is a power-of-two multiple of an fp32 number and
    x 2^T - hi is the residual of a rounding: both are exact before their own single rounding, which is what float64 gives here.
    The kernel forms both products as FMAs with a +0 addend; that shows in one place, the sign of a zero: a -0 input gives +0 planes
    (-0 + +0 = +0), while a negative value that underflows to zero in fp16 stays -0.  The `+ 0.0` below are those addends."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    xs = np.ldexp(x, range_exponent(bound)) + 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        hi = xs.astype(np.float16)
        rest = (xs - hi.astype(np.float64)).astype(np.float32)
        lo = (np.ldexp(rest.astype(np.float64), 11) + 0.0).astype(np.float16)
    return hi, lo


def wgrad_split(x, dz, khw, stride, x_bound, z_bound, x_scale=1.0):
    """the split-operand weight gradient of ONE source (csrc/wgrad_x3.hip), [kh, kw, Cx, Cout] in float64:
        x_scale 2^-(Tx + Tz) (sum Xh Zh + 2^-11 sum (Xl Zh + Xh Zl)),   X 2^Tx = Xh + Xl 2^-11,  dZ 2^Tz = Zh + Zl 2^-11
    -- the Xl Zl 2^-22 term is dropped, as the kernel drops it."""
    xh, xl = (p.astype(np.float64) for p in split_planes(x, x_bound))
    zh, zl = (p.astype(np.float64) for p in split_planes(dz, z_bound))
    shape = tuple(khw) + (xh.shape[3], zh.shape[3])
    hi = wgrad(xh, None, zh, shape, stride, 1.0, None)
    lo = wgrad(xl, None, zh, shape, stride, 1.0, None) + wgrad(xh, None, zl, shape, stride, 1.0, None)
    return float(x_scale) * np.ldexp(hi + np.ldexp(lo, -11), -(range_exponent(x_bound) + range_exponent(z_bound)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the split-operand forward model (csrc/conv_x3.hip, conv_x3n.hip), for tests/test_gpu_conv_x3_exact.py
# ---------------------------------------------------------------------------------------------------------------------------------
def weight_exponent(w, x2_scale=1.0):
    """S of shdr::weight_scale (csrc/split.h; x3_pack_kernel and x3n_pack_kernel call it): 14 - (frexp exponent of max(max |w| max(1, |x2_scale|), 1e-30)), the product formed in fp32;
    clamped to +-100.  2^S brings the largest filter element to [2^13, 2^14)."""
    f = np.float32
    mx = f(np.abs(np.asarray(w, dtype=np.float32)).max(initial=f(0.0))) * max(f(1.0), abs(f(x2_scale)))
    mx = max(f(mx), f(1e-30))
    _, ex = np.frexp(np.float64(mx))
    return int(min(max(14 - int(ex), -100), 100))


def weight_planes(w, c1, x2_scale=1.0):
    """(S, wh, ws, wl) of an HWIO filter as the pack kernels state them, the planes fp16 numbers held in float64:
    v = fp32(w 2^S), rows >= c1 one more fp32 product with x2_scale; wh = fp16(v), wl = fp16(v - wh), ws = fp16(wh 2^-11) -- an fp16
    product (v_pk_mul_f16), which underflows gradually below |wh| = 2^-3."""
    w = np.asarray(w, dtype=np.float32)
    s = weight_exponent(w, x2_scale)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.ldexp(w.astype(np.float64), s).astype(np.float32)
        if c1 < w.shape[2]:
            v[:, :, c1:] = (v[:, :, c1:].astype(np.float64) * np.float64(np.float32(x2_scale))).astype(np.float32)
        v = v.astype(np.float64)
        wh = v.astype(np.float16)
        wl = (v - wh.astype(np.float64)).astype(np.float32).astype(np.float16)
        ws = np.ldexp(wh.astype(np.float64), -11).astype(np.float16)
    return s, wh.astype(np.float64), ws.astype(np.float64), wl.astype(np.float64)


def common_lsb(*arrays):
    """the largest power of two of which every element of every array is an integer multiple (elements: multiples of 2^-40 below
    2^23; 1.0 for arrays without a non-zero element)"""
    bits = 0
    for a in arrays:
        q = np.ldexp(np.abs(np.asarray(a, dtype=np.float64)), 40)
        assert np.array_equal(q, np.rint(q)) and float(q.max(initial=0.0)) < 2.0 ** 63, "common_lsb: value off the 2^-40 grid"
        bits |= int(np.bitwise_or.reduce(q.astype(np.uint64).reshape(-1), initial=np.uint64(0)))
    return 1.0 if bits == 0 else float(bits & -bits) * 2.0 ** -40


def conv_split(x, x2, w, bias, stride, x2_scale, x_bound, x2_bound=None, pad=None, out_hw=None):
    """the split-operand convolution as conv_x3_kernel / conv_x3_1x1_kernel / conv_x3n_kernel compute it, in float64:
        T = range_exponent(the larger of the two bounds)   (shdr::range_scale, csrc/split.h: ONE scale for both sources)
        (xh, xl) = split_planes(concat[x, x2], that bound)  (the second source enters UNSCALED: its scale lives in the filter planes)
        acc = conv(xh, wh) + conv(xl, ws) + conv(xh, wl)    (three MFMAs into one fp32 accumulator; xl wl 2^-11 is dropped)
        z   = acc 2^-(S + T) + bias
    Returns (z, sum of |terms| per output, common lsb of the terms), the last two in units of the accumulator: where
    sum / lsb < 2^24 the fp32 accumulator holds every partial sum exactly, in any order."""
    c1 = np.asarray(x).shape[-1]
    xin = _sources(x, x2, 1.0)
    bits = lambda b: int(np.asarray(b, dtype=np.float32).view(np.uint32))      # the kernel compares the slots' bit patterns, unsigned
    bound = x_bound if x2 is None or bits(x_bound) >= bits(x2_bound) else x2_bound
    t = range_exponent(bound)
    xh, xl = (p.astype(np.float64) for p in split_planes(xin, bound))
    s, wh, ws, wl = weight_planes(w, c1, x2_scale if x2 is not None else 1.0)
    kw = dict(stride=stride, x2_scale=1.0, pad=pad, out_hw=out_hw)
    pairs = [(p, q) for p, q in ((xh, wh), (xl, ws), (xh, wl)) if p.any() and q.any()]          # (an empty plane contributes nothing)
    acc, total = 0.0, 0.0
    for p, q in pairs:
        acc = acc + conv2d(p, None, q, None, **kw)
        total = total + conv2d(np.abs(p), None, np.abs(q), None, **kw)
    if not pairs:
        acc = total = conv2d(xh, None, wh, None, **kw)
    groups = [slice(0, c1)] + ([slice(c1, xin.shape[-1])] if x2 is not None else [])           # (the sources differ in scale: an lsb per source)
    lsb = min([common_lsb(p[..., g]) * common_lsb(q[:, :, g]) for p, q in pairs for g in groups if p[..., g].any() and q[:, :, g].any()] or [1.0])
    z = np.ldexp(acc, -(s + t))
    if bias is not None:
        z = z + np.asarray(bias, dtype=np.float64)[:z.shape[-1]]
    return z, total, lsb


def resize2x(x):
    """tf.image.resize(x, 2x, BILINEAR) with half-pixel centres in the order of resize2x_kernel and of conv_x3_kernel's expand_store:
    horizontal first, then vertical, each a + (b - a) w with w = 0.25 (odd output index: neighbours m, m + 1) or 0.75 (even: m - 1, m),
    edges clamped.  Computed in the dtype of x: float64 for the pin against the oracle, float32 with one rounding per operation."""
    x = np.asarray(x)
    dt = x.dtype.type

    def lerp(a, axis):
        n = a.shape[axis]
        i = np.arange(2 * n)
        m = i >> 1
        odd = (i & 1) == 1
        ia = np.where(odd, m, np.maximum(m - 1, 0))
        ib = np.where(odd, np.minimum(m + 1, n - 1), m)
        wgt = np.where(odd, dt(0.25), dt(0.75)).astype(x.dtype)
        shape = [1] * a.ndim
        shape[axis] = 2 * n
        va, vb = np.take(a, ia, axis=axis), np.take(a, ib, axis=axis)
        return (va + ((vb - va).astype(x.dtype) * wgt.reshape(shape)).astype(x.dtype)).astype(x.dtype)
    return lerp(lerp(x, 2), 1)


def _windows(y):
    y = np.asarray(y, dtype=np.float32)
    assert y.shape[1] % 2 == 0 and y.shape[2] % 2 == 0
    return y[:, 0::2, 0::2], y[:, 0::2, 1::2], y[:, 1::2, 0::2], y[:, 1::2, 1::2]


def maxpool2(y):
    """MaxPool2D(2) of an fp32 tensor"""
    tl, tr, bl, br = _windows(y)
    return np.maximum(np.maximum(tl, bl), np.maximum(tr, br))


def avgpool2(y):
    """AveragePooling2D(2) in fp32 as the kernels add: 0.25 ((top-left + top-right) + (bottom-left + bottom-right)), each step rounded"""
    tl, tr, bl, br = _windows(y)
    return (np.float32(0.25) * ((tl + tr).astype(np.float32) + (bl + br).astype(np.float32)).astype(np.float32)).astype(np.float32)


def project(y, proj):
    """(sum_c proj[j][c] y[..., c], sum_c |proj[j][c] y[..., c]|) in float64: the projected output of shdr_conv2d_fwd_x3_projected_f32"""
    y = np.asarray(y, dtype=np.float64)
    p = np.asarray(proj, dtype=np.float64)
    return y @ p.T, np.abs(y) @ np.abs(p).T


# ---------------------------------------------------------------------------------------------------------------------------------
# the low-resolution channel mix of the up-sampling 3x3 layers (csrc/up2_lowres.hip), for tests/test_gpu_up2_lowres_exact.py
# (DESIGN.md section 4.6): what the two launches compute, not the ideal layer
# ---------------------------------------------------------------------------------------------------------------------------------
def up2_lowres_columns(cout, pad=None):
    """columns of z (z_columns): 9 Cout rounded up to 256 where that pads at most an eighth, else to 128; `pad` = 128 | 256 forces one, as
    SHDR_UP2_LOWRES_PAD does"""
    cols = 9 * cout
    c128, c256 = -(-cols // 128) * 128, -(-cols // 256) * 256
    if pad is not None:
        return c256 if int(pad) == 256 else c128
    return c256 if (c256 - cols) * 8 <= cols else c128


def up2_lowres_filter(w, cp):
    """st[0, 0, ci, t Cout + co] = w[ty, tx, ci, co], t = 3 ty + tx (up2_lowres_filter_kernel); columns >= 9 Cout are zero"""
    w = np.asarray(w, dtype=np.float64)
    kh, kw, cin, cout = w.shape
    assert (kh, kw) == (3, 3) and cp >= 9 * cout
    st = np.zeros((1, 1, cin, cp))
    st[0, 0, :, :9 * cout] = w.reshape(9, cin, cout).transpose(1, 0, 2).reshape(cin, 9 * cout)
    return st


def _bilinear_taps(n, t):
    """per hi-res output index r of 2n and tap t of three: (inside, ia, wa, ib, wb) -- the hi-res cell q = r + t - 1 the tap reads, whether
    it lies inside [0, 2n), and its two low-res neighbours with the half-pixel weights of resize2x (indices clamped)"""
    q = np.arange(2 * n) + t - 1
    inside = (q >= 0) & (q < 2 * n)
    qc = np.clip(q, 0, 2 * n - 1)
    m, odd = qc >> 1, (qc & 1) == 1
    ia = np.where(odd, m, np.maximum(m - 1, 0))
    ib = np.where(odd, np.minimum(m + 1, n - 1), m)
    return inside, ia, np.where(odd, 0.75, 0.25), ib, np.where(odd, 0.25, 0.75)


def up2_lowres_stencil(z, cout):
    """(y, A) of up2_lowres_stencil_kernel before its epilogue, z [N, h, w, >= 9 Cout] the tap planes:
        y[r, s, c] = sum_t [tap inside 2h x 2w] sum_{m, j} B_{r+ty-1}(m) B_{s+tx-1}(j) z[m, j, t Cout + c]
    B the half-pixel bilinear weights with clamped indices; A the same sum over |z| (every weight is >= 0).  The cells are gathered, not
    multiplied by zero weights: a NaN of z reaches exactly the outputs whose taps read it."""
    z = np.asarray(z, dtype=np.float64)
    n, h, w = z.shape[:3]
    y = np.zeros((n, 2 * h, 2 * w, cout))
    a = np.zeros_like(y)
    for ty in range(3):
        rin, *rows = _bilinear_taps(h, ty)
        for tx in range(3):
            sin, *cols = _bilinear_taps(w, tx)
            zt = z[..., (3 * ty + tx) * cout:(3 * ty + tx + 1) * cout]
            inside = (rin[:, None] & sin[None, :])[None, :, :, None]
            for ri, rw in (rows[0:2], rows[2:4]):
                for si, sw in (cols[0:2], cols[2:4]):
                    g = zt[:, ri][:, :, si] * (rw[:, None] * sw[None, :])[None, :, :, None]
                    y += np.where(inside, g, 0.0)
                    a += np.where(inside, np.abs(g), 0.0)
    return y, a


def up2_lowres(x, bound, w, pad=None):
    """the layer as csrc/up2_lowres.hip computes it: conv_split of the LOW-RES x with the restaged 1x1 filter (launch A), then the stencil
    (launch B).  Returns (z [N, h, w, Cp], y [N, 2h, 2w, Cout], gemm, stencil): gemm = max sum |terms| / lsb of the GEMM's accumulator,
    stencil = max A / (lsb_z / 16) with lsb_z = lsb 2^-(S + T).  Every stencil weight is a multiple of 1 / 16 (the horizontal ones of
    1 / 4), so the terms of one output share that lsb; below 2^24 every fp32 partial sum of the pass is exact, the horizontal sums H
    included (|H| <= 4 A in units four times as coarse)."""
    cout = np.asarray(w).shape[3]
    st = up2_lowres_filter(w, up2_lowres_columns(cout, pad))
    z, total, lsb = conv_split(x, None, st, None, 1, 1.0, bound)
    lsb_z = lsb * 2.0 ** -(weight_exponent(st) + range_exponent(bound))
    y, a = up2_lowres_stencil(z, cout)
    return z, y, float(total.max()) / lsb, float(a.max()) / (lsb_z / 16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact-fp32 kernels (csrc/conv.hip, winograd.hip, winograd_fused.hip, the input-gradient plumbing of conv_plan.hip), for
# tests/test_gpu_conv_f32_exact.py: Winograd F(2x2, 3x3) by its definition, bf16 rounding, the packed filter
# ---------------------------------------------------------------------------------------------------------------------------------
WINO_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
WINO_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
WINO_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def to_bf16(v):
    """round to the nearest bfloat16, ties to even, returned in float64: the upper 16 bits of the fp32 word after adding 0x7FFF + (bit
    16).  The fp32 subnormals round the same way (bf16 shares fp32's exponent range); values beyond the largest bf16 become infinity."""
    with np.errstate(over="ignore"):
        a = np.ascontiguousarray(v, dtype=np.float64).astype(np.float32)
    assert not np.isnan(a).any()
    b = a.view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return b.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(v))


def winograd_filter(w):
    """U[xi = 4 i + j][ci][co] = (G g G^T)[i][j] of a 3x3 HWIO filter (winograd_filter_kernel)"""
    w = np.asarray(w, dtype=np.float64)
    assert w.shape[:2] == (3, 3)
    return np.einsum("ia,abco,jb->ijco", WINO_G, w, WINO_G).reshape(16, w.shape[2], w.shape[3])


def winograd_rows(n, h, w):
    """(tiles, rows of a V / M plane): N ceil(H / 2) ceil(W / 2), and that rounded up to the 128-row GEMM tile (shdr_winograd_tiles)"""
    t = n * ((h + 1) // 2) * ((w + 1) // 2)
    return t, -(-t // 128) * 128


def winograd_input(x):
    """V[xi = 4 i + j][t][c] = (B^T d B)[i][j], d the 4x4 patch at (2 th - 1, 2 tw - 1) of tile t = (n TH + th) TW + tw, zero outside
    the image (winograd_input_kernel); the planes carry the tiles only, not the padding rows"""
    x = np.asarray(x, dtype=np.float64)
    n, h, w, c = x.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = np.zeros((n, 2 * th + 2, 2 * tw + 2, c))
    xp[:, 1:h + 1, 1:w + 1] = x
    d = np.stack([np.stack([xp[:, i:i + 2 * th:2, j:j + 2 * tw:2] for j in range(4)]) for i in range(4)])       # [4, 4, n, th, tw, c]
    return np.einsum("ia,abntwc,jb->ijntwc", WINO_BT, d, WINO_BT).reshape(16, n * th * tw, c)


def winograd_output(m, n, h, w):
    """Y = A^T M A per tile, m [16][tiles][C] -> [N, H, W, C] (the cells of a half tile beyond an odd H or W are dropped)"""
    m = np.asarray(m, dtype=np.float64)
    th, tw = (h + 1) // 2, (w + 1) // 2
    c = m.shape[2]
    y = np.einsum("ia,abntwc,jb->ntiwjc", WINO_AT, m.reshape(4, 4, n, th, tw, c), WINO_AT).reshape(n, 2 * th, 2 * tw, c)
    return y[:, :h, :w]


def winograd_conv(x, x2, w):
    """the 3x3 / stride-1 / SAME convolution of concat[x, x2] in the Winograd domain, float64: (y, gemm, out) with
        gemm = max over (xi, tile, cout) of sum_c |V| |U| / lsb,   out = max over (tile, cout) of sum_xi |M| / lsb,   lsb = lsb(V) lsb(U)
    -- where both are below 2^24 the fp32 sums over the channels (in any order, chunk by chunk) and the 16-term output transform are
    exact, every intermediate being a multiple of lsb: the kernels must then reproduce the direct convolution bit for bit."""
    xin = _sources(x, x2, 1.0)
    n, h, wd, _ = xin.shape
    v, u = winograd_input(xin), winograd_filter(w)
    m = np.einsum("xtc,xco->xto", v, u)
    lsb = common_lsb(v) * common_lsb(u)
    gemm = float(np.einsum("xtc,xco->xto", np.abs(v), np.abs(u)).max()) / lsb
    out = float(np.abs(m).sum(axis=0).max()) / lsb
    return winograd_output(m, n, h, wd), gemm, out


def winograd_packed_index(cin, cout):
    """idx[xi][ci][co] = offset of U[xi][ci][co] in the operand order of winograd_fused_kernel (winograd_filter_packed_kernel):
        ((((pn 8 + w8) nch + c) 4 + j) 64 + lane) 4 + nt,   pn = co >> 6, w8 = xi >> 1, nch = Cin / 8, c = ci >> 3,
        j = 2 (xi & 1) + (ci & 1), lane = 16 ((ci & 7) >> 1) + (co & 15), nt = (co & 63) >> 4
    -- a bijection onto [0, 16 Cin Cout) for Cin % 8 == 0 and Cout % 64 == 0"""
    assert cin % 8 == 0 and cout % 64 == 0
    xi, ci, co = np.meshgrid(np.arange(16), np.arange(cin), np.arange(cout), indexing="ij")
    nch = cin // 8
    j = 2 * (xi & 1) + (ci & 1)
    lane = 16 * ((ci & 7) >> 1) + (co & 15)
    return ((((((co >> 6) * 8 + (xi >> 1)) * nch + (ci >> 3)) * 4 + j) * 64 + lane) * 4 + ((co & 63) >> 4)).astype(np.int64)
