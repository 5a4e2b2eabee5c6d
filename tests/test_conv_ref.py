"""tests/conv_ref.py (the float64 reference of tests/test_gpu_fp16_conv_exact.py and tests/test_gpu_wgrad_f32_exact.py) pinned at 1e-12 on
random float64 inputs:
conv2d to oracle.ops.conv2d, dgrad / wgrad to float64 autograd through tests/torch_ref.py::conv2d, the explicit pad / out_hw form to
the polyphase decomposition of the stride-2 input gradient; the helpers of the fp32 weight-gradient tests (bias_grad, filter_transform,
range_exponent, split_planes, wgrad_split) to their definitions."""
import numpy as np
import pytest
import torch

import conv_ref as C
import torch_ref as R
from oracle import ops

TOL = 1e-12

# n, h, w, c1, c2, cout, k, stride, x2_scale
CASES = [
    (2, 7, 9, 5, 0, 4, 1, 1, 1.0),
    (1, 8, 8, 3, 0, 6, 3, 1, 1.0),
    (2, 7, 5, 4, 3, 5, 3, 1, 1.0 / 255),
    (1, 9, 6, 2, 0, 3, 5, 1, 1.0),
    (1, 11, 10, 3, 2, 2, 7, 1, 0.25),
    (2, 8, 8, 4, 0, 3, 1, 2, 1.0),
    (2, 7, 9, 4, 0, 3, 1, 2, 1.0),
    (1, 8, 10, 3, 0, 4, 3, 2, 1.0),
    (2, 7, 9, 3, 2, 4, 3, 2, 2.0 ** -8),
    (1, 10, 8, 2, 0, 3, 5, 2, 1.0),
    (1, 12, 12, 2, 0, 3, 7, 2, 1.0),
    (1, 13, 11, 2, 3, 2, 7, 2, 0.5),
    (1, 1, 1, 3, 0, 2, 3, 1, 1.0),
]
IDS = ["%dx%dx%d_%d+%d_%d_k%ds%d" % c[:8] for c in CASES]


def operands(case):
    n, h, w, c1, c2, cout, k, stride, x2s = case
    rng = np.random.default_rng(h * 31 + w * 7 + k)
    x = rng.normal(size=(n, h, w, c1))
    x2 = rng.normal(size=(n, h, w, c2)) / x2s if c2 else None
    wt = rng.normal(size=(k, k, c1 + c2, cout))
    b = rng.normal(size=cout)
    dz = rng.normal(size=(n, -(-h // stride), -(-w // stride), cout))
    return x, x2, wt, b, dz


def close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float(np.abs(a - b).max()) <= TOL * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv2d_matches_the_numpy_oracle(case):
    x, x2, wt, b, _ = operands(case)
    xin = x if x2 is None else np.concatenate([x, x2 * case[8]], -1)
    close(C.conv2d(x, x2, wt, b, case[7], case[8]), ops.conv2d(xin, wt, b, case[7]))
    close(C.conv2d(x, x2, wt, None, case[7], case[8]), ops.conv2d(xin, wt, None, case[7]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dgrad_and_wgrad_match_float64_autograd(case):
    n, h, w, c1, c2, cout, k, stride, x2s = case
    x, x2, wt, b, dz = operands(case)
    tx, tw = R.T(x, True), R.T(wt, True)
    tx2 = R.T(x2, True) if c2 else None
    xin = tx if tx2 is None else torch.cat([tx, tx2 * x2s], -1)
    (R.conv2d(xin, tw, R.T(b), stride) * R.T(dz)).sum().backward()
    close(C.dgrad(dz, wt, x.shape, 0, c1, 1.0, stride), tx.grad.numpy())
    if c2:
        close(C.dgrad(dz, wt, x2.shape, c1, c2, x2s, stride), tx2.grad.numpy())
    close(C.wgrad(x, x2, dz, wt.shape, stride, x2s, None), tw.grad.numpy())
    # cout_valid: the columns beyond it are zero, the others unchanged; dz channels beyond the filter's columns carry no input gradient
    cv = max(cout - 1, 1)
    dw = C.wgrad(x, x2, dz, wt.shape, stride, x2s, cv)
    close(dw[..., :cv], tw.grad.numpy()[..., :cv])
    assert not dw[..., cv:].any()
    close(C.dgrad(np.concatenate([dz, dz], -1), wt, x.shape, 0, c1, 1.0, stride), tx.grad.numpy())


def filter_transform(wt, c_begin, c_count, scale):
    """the filter of the input gradient written as a forward conv on dz: flipped taps, rows and columns exchanged"""
    return scale * np.ascontiguousarray(wt[::-1, ::-1, c_begin:c_begin + c_count, :].transpose(0, 1, 3, 2))


@pytest.mark.parametrize("case", [c for c in CASES if c[7] == 1], ids=[i for c, i in zip(CASES, IDS) if c[7] == 1])
def test_stride1_input_gradient_is_a_same_conv_with_the_flipped_filter(case):
    n, h, w, c1, c2, cout, k, stride, x2s = case
    x, x2, wt, b, dz = operands(case)
    close(C.conv2d(dz, None, filter_transform(wt, 0, c1, 1.0), None, 1, 1.0), C.dgrad(dz, wt, x.shape, 0, c1, 1.0, 1))


@pytest.mark.parametrize("case", [c for c in CASES if c[7] == 2 and c[6] > 1], ids=[i for c, i in zip(CASES, IDS) if c[7] == 2 and c[6] > 1])
def test_explicit_pad_form_composes_the_polyphase_input_gradient(case):
    """conv2d with explicit pad / out_hw on the four sub-sampled flipped filters (the decomposition of the product's stride-2 input
    gradient) reproduces the autograd-pinned dgrad"""
    n, h, w, c1, c2, cout, k, stride, x2s = case
    x, x2, wt, b, dz = operands(case)
    filt = filter_transform(wt, 0, c1, 1.0)
    _, pt = C.same_pad(h, k, 2)
    _, pl = C.same_pad(w, k, 2)

    def phase(par_in, pad_fwd):
        par = (par_in + pad_fwd) % 2
        taps = len(range(par, k, 2))
        off = (par_in + pad_fwd - par) // 2
        return k - 1 - par - 2 * (taps - 1), taps - 1 - off, taps
    dx = np.zeros((n, h, w, c1))
    for p in range(2):
        a0, pad_t, th = phase(p, pt)
        mh = (h - p + 1) // 2
        for q in range(2):
            b0, pad_l, tw = phase(q, pl)
            mw = (w - q + 1) // 2
            if mh == 0 or mw == 0 or th == 0 or tw == 0:
                continue
            dx[:, p::2, q::2] = C.conv2d(dz, None, filt[a0::2, b0::2], None, 1, 1.0, pad=(pad_t, pad_l), out_hw=(mh, mw))
    close(dx, C.dgrad(dz, wt, x.shape, 0, c1, 1.0, 2))


def test_epilogue_order_and_roundings():
    z = np.array([[-3.0, 5.0, -20.0, 7.0]])
    f = np.float32
    # leaky relu: one fp32 product with the fp32 constant, not the float64 product
    got = C.epilogue(z, C.ACT_LRELU)
    assert got.dtype == np.float32 and got[0, 0] == f(-3.0) * f(0.1) and got[0, 1] == 5.0
    # act1, scale, shift, residual, act2 -- in that order
    got = C.epilogue(z, C.ACT_RELU, scale=[2, 2, 2, 0.5], shift=[1, -20, 1, 1], residual=np.array([[0.0, 2.0, -3.0, 0.5]]), act2=C.ACT_RELU)
    np.testing.assert_array_equal(got, np.array([[1.0, 0.0, 0.0, 5.0]], dtype=np.float32))
    # residual channels beyond the output's are ignored (res_cstride > channels)
    np.testing.assert_array_equal(C.epilogue(z[:, :2], C.ACT_NONE, residual=np.array([[1.0, 1.0, 9.0]])), np.array([[-2.0, 6.0]], dtype=np.float32))


def test_to_f16_rounds_once_to_nearest_even():
    got = C.to_f16(np.array([2049.0, 2051.0, 2050.0, -2049.0, 0.1]))
    np.testing.assert_array_equal(got.astype(np.float64), [2048.0, 2052.0, 2050.0, -2048.0, float(np.float16(0.1))])
    # one rounding: 2049 + 2^-20 lies above the tie and goes up, although its fp32 rounding (2049) would go down
    assert float(C.to_f16(2049.0 + 2.0 ** -20)) == 2050.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the helpers of the fp32 weight-gradient tests (tests/test_gpu_wgrad_f32_exact.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bias_grad_is_the_pixel_sum():
    dz = np.random.default_rng(3).normal(size=(2, 5, 7, 6))
    close(C.bias_grad(dz), np.einsum("nhwc->c", dz))
    close(C.bias_grad(dz[0, 0]), dz[0, 0].sum(0))


@pytest.mark.parametrize("case", [c for c in CASES if c[7] == 1], ids=[i for c, i in zip(CASES, IDS) if c[7] == 1])
def test_filter_transform_then_conv2d_is_the_input_gradient(case):
    """every source of the layer: c_begin > 0, c_count < Cin and the scale of the second source included"""
    n, h, w, c1, c2, cout, k, stride, x2s = case
    x, x2, wt, b, dz = operands(case)
    close(C.filter_transform(wt, 0, c1, 1.0), filter_transform(wt, 0, c1, 1.0))
    close(C.conv2d(dz, None, C.filter_transform(wt, 0, c1, 1.0), None, 1, 1.0), C.dgrad(dz, wt, x.shape, 0, c1, 1.0, 1))
    if c2:
        close(C.conv2d(dz, None, C.filter_transform(wt, c1, c2, x2s), None, 1, 1.0), C.dgrad(dz, wt, x2.shape, c1, c2, x2s, 1))


def test_filter_transform_indices_on_a_non_square_filter():
    w = np.arange(3 * 4 * 5 * 2, dtype=np.float64).reshape(3, 4, 5, 2)
    wt = C.filter_transform(w, 1, 3, 0.5)
    assert wt.shape == (3, 4, 2, 3)
    for kh, kw, co, ci in ((0, 0, 0, 0), (2, 3, 1, 2), (1, 2, 1, 0), (0, 3, 0, 1)):
        assert wt[kh, kw, co, ci] == 0.5 * w[2 - kh, 3 - kw, 1 + ci, co]


def test_range_exponent():
    f = np.float32
    assert C.range_exponent(2.0) == 9 and C.range_exponent(1.0) == 10 and C.range_exponent(np.nextafter(f(1.0), f(0.0))) == 11
    assert C.range_exponent(1024.0) == 0 and C.range_exponent(2047.9) == 0 and C.range_exponent(2048.0) == -1
    for b in (2.0, 1.7, 3e-8, 6e4, 1e-30, 1e30):
        assert 2.0 ** 10 <= float(f(b)) * 2.0 ** C.range_exponent(b) < 2.0 ** 11
    # no bound in the slot
    assert C.range_exponent(0.0) == 0 and C.range_exponent(np.inf) == 0 and C.range_exponent(np.nan) == 0
    assert C.range_exponent(-0.0) == 0 and C.range_exponent(-3.0) == 0 and C.range_exponent(np.uint32(0x7FC5A5A5).view(f)) == 0
    # clamps: denormal and tiny bounds; the largest finite bound stays above the lower one
    assert C.range_exponent(np.uint32(1).view(f)) == 126 and C.range_exponent(2.0 ** -116) == 126 and C.range_exponent(2.0 ** -115) == 125
    assert C.range_exponent(np.finfo(f).max) == -117


def test_split_planes_recombine_within_the_documented_bound():
    """|x 2^T - (hi + lo 2^-11)| <= 3 * 2^-22 |x 2^T| (csrc/wgrad_x3.hip) on random fp32 data over eight decades, the slot holding the
    tensor's own maximum; both planes are fp16 numbers, and the high plane alone is the fp16 rounding of the scaled tensor"""
    rng = np.random.default_rng(17)
    x = (rng.normal(size=20000) * np.exp(4.0 * rng.normal(size=20000))).astype(np.float32)
    for scale in (1.0, 3e-8, 2e4):
        xs = (x * np.float32(scale)).astype(np.float32)
        bound = np.abs(xs).max()
        hi, lo = C.split_planes(xs, bound)
        assert hi.dtype == np.float16 and lo.dtype == np.float16 and np.isfinite(hi).all() and np.isfinite(lo).all()
        t = C.range_exponent(bound)
        want = np.ldexp(xs.astype(np.float64), t)
        assert float(np.abs(want).max()) < 2048.0
        np.testing.assert_array_equal(hi, want.astype(np.float16))
        err = np.abs(want - (hi.astype(np.float64) + np.ldexp(lo.astype(np.float64), -11)))
        normal = np.abs(want) >= 2.0 ** -14                                # (below: fp16 denormals, absolute bound 2^-24 * 2^-11)
        assert (err[normal] <= 3 * 2.0 ** -22 * np.abs(want[normal])).all()
        assert (err[~normal] <= 2.0 ** -36).all()


def test_split_planes_ties_zeros_and_empty_slots():
    f = np.float32
    # stated in the scaled domain (slot 1024 -> T = 0): ties go to the even neighbour, the rest keeps its sign
    x = np.array([1024.5, 1025.5, 2.0 + 2.0 ** -11, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 0.0, -0.0, 2.0 ** -25, -1024.5,
                  -2.0 ** -26, -2.0 ** -40], dtype=f)
    hi, lo = C.split_planes(x, 1024.0)
    np.testing.assert_array_equal(hi.astype(np.float64), [1024.0, 1026.0, 2.0, 1.0, 1.0 + 2.0 ** -9, 0.0, 0.0, 0.0, -1024.0, 0.0, 0.0])
    np.testing.assert_array_equal(lo.astype(np.float64), [1024.0, -1024.0, 1.0, 1.0, -1.0, 0.0, 0.0, 2.0 ** -14, -1024.0, -2.0 ** -15, 0.0])
    # signs of zeros, as the kernel's FMAs with a +0 addend leave them: a -0 input gives +0 planes; a negative value that underflows
    # keeps its sign (hi of -2^-26; both planes of -2^-40)
    assert not np.signbit(hi[[5, 6, 7]]).any() and not np.signbit(lo[[5, 6]]).any()
    assert np.signbit(hi[[9, 10]]).all() and np.signbit(lo[10])
    # a slot without a bound leaves the tensor unscaled
    for empty in (0.0, np.inf, np.nan):
        h2, l2 = C.split_planes(x, empty)
        np.testing.assert_array_equal(h2.view(np.uint16), hi.view(np.uint16))
        np.testing.assert_array_equal(l2.view(np.uint16), lo.view(np.uint16))
    # scaling is exact: the planes of x 2^-9 under the slot 2.0 are the planes of x under 1024
    h3, l3 = C.split_planes(np.ldexp(x, -9), 2.0)
    np.testing.assert_array_equal(h3.view(np.uint16), hi.view(np.uint16))
    np.testing.assert_array_equal(l3.view(np.uint16), lo.view(np.uint16))


@pytest.mark.parametrize("low_plane_of", ["x", "dz"])
@pytest.mark.parametrize("k,stride", [(3, 1), (7, 2), (1, 1)])
def test_wgrad_split_is_exact_when_one_low_plane_is_empty(low_plane_of, k, stride):
    """X 2^Tx = Xh + Xl 2^-11 with Zl = 0 (or the other way round): the dropped term Xl Zl is zero and the model IS the weight gradient"""
    rng = np.random.default_rng(k * 5 + stride)
    n, h, w, cx, cout = 2, 9, 11, 5, 4
    kk = rng.choice([-2.0, 2.0], size=(n, h, w, cx))
    jj = rng.integers(-1, 2, size=(n, h, w, cx)) * np.sign(kk) + (rng.integers(0, 2, size=(n, h, w, cx)) * np.sign(kk))
    fine = np.ldexp(kk + np.ldexp(jj, -11), -7)                           # slot 8.0 -> T = 7
    ho, wo = -(-h // stride), -(-w // stride)
    if low_plane_of == "x":
        x, dz, xb, zb = fine, rng.integers(-2, 3, size=(n, ho, wo, cout)).astype(np.float64), 8.0, 2.0
    else:
        x = rng.integers(-2, 3, size=(n, h, w, cx)).astype(np.float64)
        dz = np.ldexp(rng.choice([-2.0, 2.0], size=(n, ho, wo, cout)) + np.ldexp(rng.integers(0, 2, size=(n, ho, wo, cout)), -11), -7)
        xb, zb = 2.0, 8.0
    hi, lo = C.split_planes(fine if low_plane_of == "x" else dz, 8.0)
    assert lo.any(), "the fine operand must have a non-empty low plane"
    eh, el = C.split_planes(dz if low_plane_of == "x" else x, 2.0)
    assert not el.any()
    want = C.wgrad(x, None, dz, (k, k, cx, cout), stride, 1.0, None)
    np.testing.assert_array_equal(C.wgrad_split(x, dz, (k, k), stride, xb, zb), want)
    np.testing.assert_array_equal(C.wgrad_split(x, dz, (k, k), stride, xb, zb, 2.0 ** -8), want * 2.0 ** -8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the split-operand forward model (tests/test_gpu_conv_x3_exact.py)
# ---------------------------------------------------------------------------------------------------------------------------------
import test_gpu_conv_x3_exact as X                                       # (no device is touched by importing it: the operand recipes live there)
import test_gpu_up2_lowres_exact as U


def test_weight_exponent_and_planes():
    f = np.float32
    assert C.weight_exponent(np.array([1.0])) == 13 and C.weight_exponent(np.array([0.999])) == 14 and C.weight_exponent(np.array([-2.0])) == 12
    assert C.weight_exponent(np.array([1.0]), 2.0 ** -8) == 13 and C.weight_exponent(np.array([1.0]), -4.0) == 11       # max(1, |x2_scale|)
    assert C.weight_exponent(np.zeros(3)) == 100 and C.weight_exponent(np.array([2.0 ** 120])) == -100 and C.weight_exponent(np.array([2.0 ** 100])) == -87
    # wh + wl == v exactly for weights down to max |w| 2^-17: the low plane of such a weight is still on the fp16 grid (2^-24 at the
    # bottom) when the weight carries 21 significant bits; a full fp32 weight (24 bits) is met to 2^-22 of itself
    rng = np.random.default_rng(5)
    w = (rng.normal(size=(3, 3, 8, 16)) * np.exp2(rng.integers(-15, 1, size=(3, 3, 8, 16)))).astype(np.float32)
    w = np.clip(w, -1.5, 1.5)
    w[0, 0, 0, 0] = 1.5
    keep = np.abs(w) >= 1.5 * 2.0 ** -17
    s, wh, ws, wl = C.weight_planes(w, 8)
    v = np.ldexp(w.astype(np.float64), s)
    assert s == 13 and keep.mean() > 0.9
    assert (np.abs(wh + wl - v)[keep] <= 2.0 ** -22 * np.abs(v)[keep]).all()
    m, e = np.frexp(w.astype(np.float64))
    w21 = np.ldexp(np.rint(np.ldexp(m, 21)), e - 21)
    w21[0, 0, 0, 0] = 1.5
    s, wh, ws, wl = C.weight_planes(w21, 8)
    v = np.ldexp(w21, s)
    assert s == 13 and np.array_equal((wh + wl)[keep], v[keep]) and (wl != 0).mean() > 0.9
    assert np.array_equal(wh, v.astype(np.float16).astype(np.float64))
    # ws is an fp16 PRODUCT: exact down to |wh| = 2^-3, gradual underflow below
    assert np.array_equal(ws[np.abs(wh) >= 0.125], np.ldexp(wh, -11)[np.abs(wh) >= 0.125])
    _, wh2, ws2, _ = C.weight_planes(np.array([[[[1.0, 2.0 ** -13 * (2.0 ** -4 + 2.0 ** -14)]]]]), 1)
    assert wh2[0, 0, 0, 1] == 2.0 ** -4 + 2.0 ** -14 and ws2[0, 0, 0, 1] == 2.0 ** -15                   # (2^-15 + 2^-25: a tie on the 2^-24 grid, to even)
    # rows >= c1 take one more fp32 product with x2_scale
    _, wh3, _, wl3 = C.weight_planes(np.ones((1, 1, 2, 1)), 1, 2.0 ** -8)
    assert wh3[0, 0, 0, 0] == 8192.0 and wh3[0, 0, 1, 0] == 32.0 and not wl3.any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv_split_is_the_convolution_when_both_low_planes_are_empty(case):
    n, h, w, c1, c2, cout, k, stride, x2s = case
    rng = np.random.default_rng(h + w)
    x, xb = X.int_x(rng, (n, h, w, c1))
    # the recipe wants a power-of-two scale (the scaled second source must stay an integer tensor): the shared case with 1 / 255 runs at 0.5
    x2s = x2s if np.frexp(x2s)[0] == 0.5 else 0.5
    x2, x2b = (X.int_x(rng, (n, h, w, c2))[0] / x2s, 2.0 / x2s) if c2 else (None, None)
    wt = X.int_w(rng, (k, k, c1 + c2, cout))
    b = rng.integers(-3, 4, size=cout).astype(np.float64)
    z, total, lsb = C.conv_split(x, x2, wt, b, stride, x2s, xb, x2b)
    np.testing.assert_array_equal(z, C.conv2d(x, x2, wt, b, stride, x2s))
    assert float(total.max()) / lsb <= 4 * k * k * (c1 + c2)
    # the explicit pad / out_hw form is handed through
    z2 = C.conv_split(x, x2, wt, b, 1, x2s, xb, x2b, pad=(0, 1), out_hw=(h, w))[0]
    np.testing.assert_array_equal(z2, C.conv2d(x, x2, wt, b, 1, x2s, pad=(0, 1), out_hw=(h, w)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv_split_stays_inside_the_documented_bound_on_gaussian_inputs(case):
    """|conv_split - conv2d| <= 3 * 2^-22 * sum |x| |w| (the bound written at the top of csrc/conv_x3.hip), bound = the measured range"""
    n, h, w, c1, c2, cout, k, stride, x2s = case
    x, x2, wt, b, _ = (None if a is None else a.astype(np.float32).astype(np.float64) for a in operands(case))
    xb = float(np.abs(x).max())
    x2b = float(np.abs(x2).max()) if c2 else None
    z = C.conv_split(x, x2, wt, b, stride, x2s, xb, x2b)[0]
    ref = C.conv2d(x, x2, wt, b, stride, x2s)
    mag = C.conv2d(np.abs(x), None if x2 is None else np.abs(x2), np.abs(wt), None, stride, abs(x2s))
    ratio = float((np.abs(z - ref) / (2.0 ** -22 * mag)).max())
    assert ratio <= 3.0, ratio
    assert ratio > 0.0, "the dropped term must show on Gaussian inputs"


def test_operand_recipes_produce_the_planes_they_promise():
    rng = np.random.default_rng(11)
    shape = (2, 9, 11, 16)
    # int: T = 9, xh = 512 x, xl empty; S = 13, wh = 8192 w, ws = 4 w, wl empty
    x, xb = X.int_x(rng, shape)
    assert xb == 2.0 and float(np.abs(x).max()) == 2.0 and C.range_exponent(xb) == 9
    xh, xl = C.split_planes(x, xb)
    assert np.array_equal(xh.astype(np.float64), 512.0 * x) and not xl.any()
    w = X.int_w(rng, (3, 3, 16, 8))
    s, wh, ws, wl = C.weight_planes(w, 16)
    assert s == 13 and np.array_equal(wh, 8192.0 * w) and np.array_equal(ws, 4.0 * w) and not wl.any()
    # fine-x: T = 7, xh = k, xl = j
    x, xb, k, j = X.fine_x(rng, shape)
    assert xb == 8.0 and C.range_exponent(xb) == 7 and j.any() and (np.abs(k) == 2).any()
    xh, xl = C.split_planes(x, xb)
    assert np.array_equal(xh.astype(np.float64), k) and np.array_equal(xl.astype(np.float64), j)
    x, xb, k, j = X.fine_x(rng, shape, kmax=1)
    assert float(np.abs(k).max()) == 1.0 and np.array_equal(C.split_planes(x, xb)[1].astype(np.float64), j)
    # fine-w: S = 13, wh = 4096 q, ws = 2 q, wl = r -- also in the rows of a second source scaled by 2^-8 (there 16 q, q 2^-7, r 2^-8)
    w, q, r = X.fine_w(rng, (3, 3, 16, 8))
    assert r.any() and not r[q == 0].any() and w[0, 0, 0, 0] == 1.0
    s, wh, ws, wl = C.weight_planes(w, 16)
    assert s == 13 and np.array_equal(wh, 4096.0 * q) and np.array_equal(ws, 2.0 * q) and np.array_equal(wl, r)
    s, wh, ws, wl = C.weight_planes(w, 8, 2.0 ** -8)
    assert s == 13 and np.array_equal(wh[:, :, 8:], 16.0 * q[:, :, 8:]) and np.array_equal(wl[:, :, 8:], r[:, :, 8:] * 2.0 ** -8)
    assert np.array_equal(ws[:, :, 8:], q[:, :, 8:] * 2.0 ** -7) and np.array_equal(wh[:, :, :8], 4096.0 * q[:, :, :8])
    # a padded head: the columns beyond it are zero
    assert not X.fine_w(rng, (3, 3, 16, 16), cols=3)[0][..., 3:].any() and not X.int_w(rng, (3, 3, 16, 16), cols=5)[..., 5:].any()


def test_fine_x_and_fine_w_together_model_the_kernel_not_the_ideal():
    """with both low planes non-empty the dropped xl wl 2^-11 term is non-zero: the reference differs from the true convolution on
    nearly every output, by exactly that term"""
    rng = np.random.default_rng(23)
    x, xb, k, j = X.fine_x(rng, (1, 9, 11, 32))
    w, q, r = X.fine_w(rng, (3, 3, 32, 16))
    z, total, lsb = C.conv_split(x, None, w, None, 1, 1.0, xb)
    ref = C.conv2d(x, None, w, None, 1, 1.0)
    assert float(total.max()) / lsb < 2.0 ** 24
    assert (z != ref).mean() > 0.9
    dropped = np.ldexp(C.conv2d(j, None, r, None, 1, 1.0), -(11 + 13 + 7))
    np.testing.assert_array_equal(ref - z, dropped)


def test_resize2x_matches_the_oracle_and_is_exact_on_integers():
    rng = np.random.default_rng(2)
    for shape in ((1, 1, 3, 2), (2, 8, 8, 3), (1, 9, 11, 4), (1, 1, 1, 1)):
        a = rng.normal(size=shape)
        close(C.resize2x(a), ops.resize_bilinear_2x(a))
        i = rng.integers(-2, 3, size=shape).astype(np.float64)
        np.testing.assert_array_equal(C.resize2x(i.astype(np.float32)).astype(np.float64), C.resize2x(i))
    # order and weights: horizontal first, a + (b - a) w with w in {0.25, 0.75}, edges clamped
    row = np.array([0.0, 4.0, 8.0]).reshape(1, 1, 3, 1)
    np.testing.assert_array_equal(C.resize2x(row)[0, 0, :, 0], [0.0, 1.0, 3.0, 5.0, 7.0, 8.0])
    assert C.resize2x(row).shape == (1, 2, 6, 1)


def test_pooled_and_projected_outputs():
    f = np.float32
    y = np.array([[1.0, -2.0, 3.0, 0.5], [4.0, 0.0, -1.0, 0.25]], dtype=f).reshape(1, 2, 4, 1)
    np.testing.assert_array_equal(C.maxpool2(y)[0, 0, :, 0], [4.0, 3.0])
    np.testing.assert_array_equal(C.avgpool2(y)[0, 0, :, 0], [0.75, 0.6875])
    # the order of the sums: (tl + tr) + (bl + br), each rounded to fp32
    big = np.array([[2.0 ** 24, 1.0], [1.0, -(2.0 ** 24)]], dtype=f).reshape(1, 2, 2, 1)
    assert C.avgpool2(big)[0, 0, 0, 0] == f(0.25) * ((f(2.0 ** 24) + f(1.0)) + (f(1.0) + f(-(2.0 ** 24))))
    y3 = np.arange(6, dtype=np.float64).reshape(1, 1, 2, 3)
    proj = np.array([[1.0, 0.0, -1.0], [2.0, 2.0, 2.0], [0.0, 0.0, 0.0]])
    yj, tj = C.project(y3, proj)
    np.testing.assert_array_equal(yj[0, 0], [[-2.0, 6.0, 0.0], [-2.0, 24.0, 0.0]])
    np.testing.assert_array_equal(tj[0, 0], [[2.0, 6.0, 0.0], [8.0, 24.0, 0.0]])
    assert C.common_lsb(np.array([0.75, 2.0]), np.array([0.0])) == 0.25 and C.common_lsb(np.zeros(3)) == 1.0


_ALL = X.X3_3X3 + X.X3_POOLED + X.X3_UP + X.XW_3X3 + X.XW_POOLED + X.XW_UP + X.X3_1X1 + X.X3_STEM + X.X3N + X.TANH


@pytest.mark.parametrize("o", _ALL)
def test_every_forward_case_meets_its_precondition_on_the_reference_alone(o):
    r = X.reference(o)
    assert r["worst"] < 1.0
    if o["mode"] == "fxw":                                               # these cases show that the test models the kernel, not the ideal
        xin = r["x"]
        ideal = C.conv2d(xin, r["x2"], r["w"], None, o["stride"], o["x2s"])
        split = C.conv_split(xin, r["x2"], r["w"], None, o["stride"], o["x2s"], r["xb"], r["x2b"])[0]
        assert (ideal != split)[..., :r["cv"]].mean() > 0.5


@pytest.mark.parametrize("o", X.DGRAD + X.DGRAD_WIDE)
def test_every_input_gradient_case_meets_its_precondition_on_the_reference_alone(o):
    X.dgrad_reference(o)


@pytest.mark.parametrize("o", X.X3N_BIG + X.X3N_BIG_OTHER)
def test_every_1056_tile_case_meets_its_precondition_on_the_reference_alone(o):
    """(the four 16 -> 16 forms share one float64 model: three of these cases cost an epilogue each)"""
    assert (o["h"] // 16) * (o["w"] // 16) == 1056 and o["mode"] == "int"
    r = X.big_reference(o) if o["c1"] == 16 and o["c2"] == 0 else X.reference(o)
    assert r["worst"] < 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the low-resolution channel mix (csrc/up2_lowres.hip): the model of tests/test_gpu_up2_lowres_exact.py
# ---------------------------------------------------------------------------------------------------------------------------------
def test_up2_lowres_columns_and_filter():
    assert [C.up2_lowres_columns(c) for c in (64, 128, 192, 256, 512)] == [640, 1280, 1792, 2304, 4608]
    assert C.up2_lowres_columns(128, 128) == 1152 and C.up2_lowres_columns(128, 256) == 1280 and C.up2_lowres_columns(64, 256) == 768
    assert C.up2_lowres_columns(64, 128) == 640 and C.up2_lowres_columns(320) == 3072
    rng = np.random.default_rng(3)
    w = rng.normal(size=(3, 3, 5, 7))
    st = C.up2_lowres_filter(w, 128)
    assert st.shape == (1, 1, 5, 128) and not st[..., 63:].any()
    for ty in range(3):
        for tx in range(3):
            np.testing.assert_array_equal(st[0, 0, :, (3 * ty + tx) * 7:(3 * ty + tx + 1) * 7], w[ty, tx])
    # one exponent S for all nine taps: that of the 3x3 filter
    for wt in (X.fine_w(rng, (3, 3, 64, 64))[0], X.int_w(rng, (3, 3, 32, 64)), rng.normal(size=(3, 3, 32, 64)) * 37.0, w * 1e-3):
        assert C.weight_exponent(C.up2_lowres_filter(wt, C.up2_lowres_columns(wt.shape[3]))) == C.weight_exponent(wt)


@pytest.mark.parametrize("shape", [(1, 1, 1, 3, 2), (1, 1, 7, 2, 3), (2, 6, 1, 3, 2), (1, 2, 2, 2, 2), (2, 5, 9, 4, 3)])
def test_up2_lowres_stencil_is_the_convolution_of_the_resized_image(shape):
    """on float64 Gaussian z = x W[t] the stencil equals conv2d(resize_bilinear_2x(x)) of the oracle at 1e-12: the algebra, zero padding
    and edge clamp included"""
    n, h, w, cin, cout = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.normal(size=(n, h, w, cin))
    wt = rng.normal(size=(3, 3, cin, cout))
    z = C.conv2d(x, None, C.up2_lowres_filter(wt, 9 * cout + 5), None, 1, 1.0)
    y, a = C.up2_lowres_stencil(z, cout)
    close(y, ops.conv2d(ops.resize_bilinear_2x(x), wt))
    close(y, C.conv2d(C.resize2x(x), None, wt, None, 1, 1.0))
    assert (a >= np.abs(y)).all() and np.array_equal(a, C.up2_lowres_stencil(np.abs(z), cout)[0])


def test_up2_lowres_in_int_mode_is_the_convolution_of_the_resized_image_exactly():
    for name, n, h, w, cin, cout in (("a", 1, 1, 1, 32, 16), ("b", 2, 3, 5, 64, 16), ("c", 1, 4, 1, 32, 8), ("d", 1, 1, 6, 32, 8)):
        x, xb, _, _, wt = X.operands("pin_ul_int_" + name, n, h, w, cin, 0, cout, 3, "int")
        z, y, gemm, stencil = C.up2_lowres(x, xb, wt)
        assert gemm < 2.0 ** 24 and stencil < 2.0 ** 24
        np.testing.assert_array_equal(y, C.conv2d(C.resize2x(x), None, wt, None, 1, 1.0))
        np.testing.assert_array_equal(z[..., :9 * cout], C.conv2d(x, None, C.up2_lowres_filter(wt, 9 * cout), None, 1, 1.0))
        assert z.shape[3] == C.up2_lowres_columns(cout) and not z[..., 9 * cout:].any()


def test_up2_lowres_stencil_carries_a_nan_to_the_taps_that_read_it_only():
    z = np.ones((1, 4, 5, 18))
    z[0, 2, 2, :] = np.nan
    mask = np.isnan(C.up2_lowres_stencil(z, 2)[0])
    hand = np.zeros((1, 8, 10, 2), dtype=bool)
    hand[0, 2:8, 2:8] = True
    assert np.array_equal(mask, hand)


@pytest.mark.parametrize("o", U.CASES + [U.RANGES_CASE, U.NAN_CASE])
def test_every_up2_lowres_case_meets_its_preconditions_on_the_reference_alone(o):
    """both ratios below 2^24 and y exact in fp32 (asserted inside U.reference); the fxw cases differ from the true layer on most outputs"""
    r = U.reference(o)
    assert r["gemm"] < 1.0 and r["stencil"] < 1.0
    assert np.array_equal(r["v"].astype(np.float32).astype(np.float64), r["v"])
    assert r["cp"] == C.up2_lowres_columns(o["cout"], o.get("pad")) and not r["z"][..., 9 * o["cout"]:].any()
    ideal = C.conv2d(C.resize2x(r["x"]), None, r["w"], None, 1, 1.0)
    if o["mode"] == "int":
        np.testing.assert_array_equal(r["v"], ideal)
    if o["mode"] == "fxw":
        assert (ideal != r["v"]).mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact-fp32 kernels (tests/test_gpu_conv_f32_exact.py): the Winograd helpers, bf16 rounding, the packed filter,
# every case's precondition, and the sensitivity of every case to the mistakes a kernel can make
# ---------------------------------------------------------------------------------------------------------------------------------
import test_gpu_conv_f32_exact as F                                      # (no device is touched by importing it)


@pytest.mark.parametrize("n,h,w,c1,c2,cout,mode", [(1, 1, 1, 8, 0, 4, "int"), (2, 5, 7, 3, 0, 2, "fx"), (1, 8, 9, 4, 4, 3, "fw"), (1, 2, 2, 2, 0, 2, "fx"),
                                                   (2, 17, 33, 8, 8, 5, "int"), (1, 16, 18, 24, 0, 3, "fw")])
def test_winograd_by_its_definition_is_the_convolution_exactly(n, h, w, c1, c2, cout, mode):
    o = F.wc("wino_pin_%d_%d_%d_%s" % (h, w, c1, mode), n, h, w, c1, c2, cout, mode=mode).values[0]
    x, x2, wt = F.operands(o)
    y, gemm, out = C.winograd_conv(x, x2, wt)
    assert gemm < F.LIMIT and out < F.LIMIT
    assert np.array_equal(y, C.conv2d(x, x2, wt, None, 1, 1.0))
    # the pieces: the plane layout of the kernels (tile t = (n TH + th) TW + tw) and the documented row count
    xin = x if x2 is None else np.concatenate([x, x2], -1)
    v, u = C.winograd_input(xin), C.winograd_filter(wt)
    tiles, rows = C.winograd_rows(n, h, w)
    assert v.shape == (16, tiles, c1 + c2) and u.shape == (16, c1 + c2, cout) and rows % 128 == 0 and 0 <= rows - tiles < 128
    th, tw = (h + 1) // 2, (w + 1) // 2
    t = ((n - 1) * th + (th - 1)) * tw + (tw - 1)                          # the last tile: its patch starts at (2 th - 3, 2 tw - 3)
    d = np.zeros((4, 4, c1 + c2))
    for i in range(4):
        for j in range(4):
            hh, ww = 2 * (th - 1) - 1 + i, 2 * (tw - 1) - 1 + j
            if 0 <= hh < h and 0 <= ww < w:
                d[i, j] = xin[n - 1, hh, ww]
    assert np.array_equal(v[:, t].reshape(4, 4, -1), np.einsum("ia,abc,jb->ijc", C.WINO_BT, d, C.WINO_BT))
    assert np.array_equal(u[5], 0.25 * wt.sum(axis=(0, 1))) and np.array_equal(u[0], wt[0, 0]) and np.array_equal(u[15], wt[2, 2])


def test_winograd_packed_index_follows_the_documented_formula():
    for cin, cout in ((8, 64), (24, 128), (72, 64)):
        idx = C.winograd_packed_index(cin, cout)
        assert idx.shape == (16, cin, cout) and np.array_equal(np.sort(idx.reshape(-1)), np.arange(16 * cin * cout))
    idx = C.winograd_packed_index(24, 128)
    nch = 3
    for xi, ci, co in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 2, 0), (0, 8, 0), (2, 0, 0), (0, 0, 16), (0, 0, 64), (15, 23, 127), (7, 13, 85)):
        pn, w8, c, j, lane, nt = co >> 6, xi >> 1, ci >> 3, 2 * (xi & 1) + (ci & 1), 16 * ((ci & 7) >> 1) + (co & 15), (co & 63) >> 4
        assert idx[xi, ci, co] == ((((pn * 8 + w8) * nch + c) * 4 + j) * 64 + lane) * 4 + nt
    assert [int(idx[a]) for a in ((1, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 16))] == [512, 256, 64, 4, 1]


def test_to_bf16_rounds_to_nearest_even_ties_and_subnormals():
    f = np.float32
    e = 2.0 ** -8                                                          # half an ulp of bf16 at 1.0 (8 significand bits)
    assert C.to_bf16([1 + e, 1 + 3 * e, 1 + e + 2.0 ** -20, 1 + e - 2.0 ** -20, -(1 + e), -(1 + 3 * e)]).tolist() == [1.0, 1 + 4 * e, 1 + 2 * e, 1.0, -1.0, -(1 + 4 * e)]
    assert C.to_bf16([0.0, -0.0, 3.0, 0.5, 255.0, 257.0, 258.0]).tolist() == [0.0, -0.0, 3.0, 0.5, 255.0, 256.0, 258.0]
    assert np.signbit(C.to_bf16(-0.0))
    # subnormals: bf16 shares fp32's exponent range; its smallest subnormal is 2^-133
    tiny = 2.0 ** -133
    assert C.to_bf16([tiny, tiny * 0.5, tiny * 0.5 + 2.0 ** -149, tiny * 1.5, tiny * 2.5, 2.0 ** -126 - 2.0 ** -149]).tolist() == \
        [tiny, 0.0, tiny, 2 * tiny, 2 * tiny, 2.0 ** -126]
    # the largest finite bf16, and the fp32 values just above it that round to infinity
    top = float(f(2.0 ** 127 * (2 - 2.0 ** -7)))
    assert C.to_bf16([top, top * (1 + 2.0 ** -10)]).tolist() == [top, top] and np.isinf(C.to_bf16(float(np.finfo(f).max)))
    # every bf16 value is a fixed point, and the rounding agrees with torch's on random words
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)
    a = words.view(f)
    a = a[np.isfinite(a)]
    want = torch.from_numpy(a.copy()).to(torch.bfloat16).to(torch.float32).numpy().astype(np.float64)
    assert np.array_equal(C.to_bf16(a.astype(np.float64)), want) and np.array_equal(C.to_bf16(want), want)
    # the recipes: rounding to fp16 or bf16 removes exactly the fine part
    x, _, k, j = F.fine_x(rng, (3, 5, 7, 4))
    assert j.any() and np.array_equal(C.to_bf16(x), np.ldexp(k, -7)) and np.array_equal(C.to_f16(x).astype(np.float64), np.ldexp(k, -7))
    wf, q, r = F.fine_w(rng, (3, 3, 4, 8))
    assert r.any() and np.array_equal(C.to_bf16(wf), q / 2) and np.array_equal(C.to_f16(wf).astype(np.float64), q / 2)


F32_FAMILIES = dict(tiles=F.TILE_CASES, geometry=F.GEOMETRY, outputs=F.OUTPUT_FORMS, epilogues=F.EPILOGUE_CASES, rega=F.REGA + F.REGA_REFUSED + F.REGA_PERSISTENT,
                    direct=F.DIRECT, prec=F.PREC)
_F32_FORWARD = [p for cases in F32_FAMILIES.values() for p in cases]


@pytest.mark.parametrize("o", _F32_FORWARD)
def test_every_f32_forward_case_meets_its_precondition_on_the_reference_alone(o):
    r = F.reference(o)
    assert r["worst"] < 1.0 and r["y"].dtype == np.float32 and np.isfinite(r["y"]).all() and r["y"].any()
    assert F.plan_expected(o) in ("mfma", "direct"), "a forward case of this file runs below the plan: no Winograd shapes here"
    if o["mode"] == "int":
        assert np.array_equal(F.model(o, *F.operands(o))[0], F.model(dict(o, algo="exact"), *F.operands(o))[0]), "int mode survives fp16 / bf16 operands"


@pytest.mark.parametrize("o", F.WINO + F.PLANES)
def test_every_winograd_case_meets_its_transform_domain_precondition(o):
    r = F.wino_reference(o)                                                # (asserts both bounds and winograd_conv == conv2d)
    assert np.isfinite(r["y"]).all() and r["y"].any()


@pytest.mark.parametrize("o", F.DGRAD)
def test_every_f32_input_gradient_case_meets_its_precondition_on_the_reference_alone(o):
    assert F.dgrad_kind(o) == o["kind"]
    dz, wt, dx, cc = F.dgrad_reference(o)
    assert dx.any() and dx.shape == (o["n"], o["h"], o["w"], cc)
    if o["kind"] == "1x1s2":
        rest = dx.copy()
        rest[:, ::2, ::2] = 0.0
        assert not rest.any()


def test_every_named_instantiation_is_reached():
    reached = {F.instance(p.values[0]) for p in _F32_FORWARD}
    want = {"conv_%s<128, %s, %s>" % (k, t, f) for k in ("mfma_dma_kernel", "mfma_kernel") for t in ("128, 2, 2", "64, 4, 1", "32, 4, 1", "16, 4, 1")
            for f in ("true", "false")}
    want |= {"conv_mfma_dma_kernel<128, %s, %s, %d>" % (t, f, p) for t in ("128, 2, 2", "64, 4, 1", "32, 4, 1", "16, 4, 1") for f in ("true", "false") for p in (1, 2)
             if (t, f) not in (("128, 2, 2", "false"), ("64, 4, 1", "false"), ("16, 4, 1", "true"))}
    want |= {"conv_rega_kernel<4, %d, %d, %d>" % (nt, ct, kk) for nt in (1, 2) for ct in (4, 16, 32) for kk in (0, 3, 5, 7) if (nt, ct, kk) != (2, 32, 7)}
    want |= {"conv_rega_kernel<4, 4, 4, 3>", "conv_direct_kernel<3>", "conv_direct_kernel<8>", "conv_direct_kernel<16>"}
    assert not want - reached, sorted(want - reached)
    # chunk counts of the LDS-DMA kernel per tile: one, two, an odd and an even >= 4 number (the 128-cout tile starts at K > 128: five)
    for tile, need in (("128, 2, 2", (5, 6, 7, 8)), ("64, 4, 1", (1, 2, 9, 4)), ("32, 4, 1", (1, 2, 9, 4)), ("16, 4, 1", (1, 2, 9, 4))):
        for kernel in ("conv_mfma_dma_kernel<128, " + tile, "conv_mfma_kernel<128, " + tile):
            chunks = set()
            for p in F.TILE_CASES:
                o = p.values[0]
                if F.instance(o).startswith(kernel):
                    ct, kk = o["c1"] + o["c2"], o["kh"] * o["kw"] * (o["c1"] + o["c2"])
                    fast = ct % 32 == 0 and (o["c2"] == 0 or o["c1"] % 32 == 0)
                    chunks.add(o["kh"] * o["kw"] * ct // 32 if fast else -(-kk // 32))
            assert set(need) <= chunks, (kernel, sorted(chunks))


def _differs(a, b):
    return a.shape != b.shape or not np.array_equal(a, b)


@pytest.mark.parametrize("family", list(F32_FAMILIES) + ["winograd", "planes"])
def test_forward_cases_tell_a_wrong_model_from_the_right_one(family):
    """every deliberately wrong model -- one tap dropped, pad off by one, the last k-chunk dropped, the two sources swapped, the right-halo
    column zeroed, operands rounded to fp16 -- changes at least one element of the expected output of EVERY case whose geometry lets it show
    (all-ones operands decide that: a 1 x 1 image reads one tap of a 3 x 3 filter, a 1x1 / 2 layer no odd column), and shows in every family: the inputs are not
    degenerate, thinning has not emptied the edge a case exists to test."""
    cases = F32_FAMILIES.get(family) or (F.WINO if family == "winograd" else F.PLANES)
    ref = F.reference if family in F32_FAMILIES else F.wino_reference
    seen = set()
    for p in cases:
        o = p.values[0]
        if o["n"] * o["h"] * o["w"] > 20000:
            continue                                                       # (the persistent-loop cases: their small twins carry the check)
        right, probe = ref(o)["y"], ref(o, probe=True)["y"]
        for wrong in F.wrong_models(o):
            if wrong in ("tap", "pad", "chunk", "halo") and not _differs(probe, ref(o, wrong=wrong, probe=True)["y"]):
                continue                                                   # this geometry cannot show it
            assert _differs(right, ref(o, wrong=wrong)["y"]), "%s: the model with '%s' gives the same output" % (p.id, wrong)
            seen.add(wrong)
    want = {"tap", "pad", "chunk", "halo", "f16"} | ({"swap"} if any(p.values[0]["c2"] for p in cases) else set())
    assert seen == want, (family, sorted(want - seen))


def test_input_gradient_cases_tell_a_wrong_model_from_the_right_one():
    seen = {}
    for p in F.DGRAD:
        o = p.values[0]
        right, probe = F.dgrad_reference(o)[2], F.dgrad_reference(o, probe=True)[2]
        for wrong in F.dgrad_wrong_models(o):
            if wrong in ("tap", "pad", "chunk", "phase") and not _differs(probe, F.dgrad_reference(o, wrong=wrong, probe=True)[2]):
                continue
            assert _differs(right, F.dgrad_reference(o, wrong=wrong)[2]), "%s: the model with '%s' gives the same gradient" % (p.id, wrong)
            seen.setdefault(o["kind"], set()).add(wrong)
    assert seen["poly"] >= {"tap", "pad", "chunk", "phase", "swap", "f16"} and seen["mfma"] >= {"tap", "pad", "chunk", "swap", "f16"}, seen
    assert seen["wino"] >= {"tap", "pad", "chunk", "swap", "f16"} and seen["1x1s2"] >= {"tap", "pad", "chunk", "f16"}, seen
