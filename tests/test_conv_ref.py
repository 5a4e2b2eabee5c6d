"""tests/conv_ref.py (the float64 reference of tests/test_gpu_fp16_conv_exact.py) pinned at 1e-12 on random float64 inputs:
conv2d to oracle.ops.conv2d, dgrad / wgrad to float64 autograd through tests/torch_ref.py::conv2d, the explicit pad / out_hw form to
the polyphase decomposition of the stride-2 input gradient."""
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
