"""tests/fp16_ref.py (the float64 reference of the fp16 tape ops, used by tests/test_gpu_fp16_elem.py) pinned at 1e-12 wherever it
overlaps oracle/ops.py and tests/torch_ref.py; its backward ops against float64 autograd."""
import numpy as np
import pytest
import torch

import fp16_ref as F
import torch_ref as R
from oracle import ops

TOL = 1e-12
SHAPES = [(1, 1, 1, 8), (1, 2, 2, 8), (1, 2, 3, 8), (2, 5, 7, 24), (1, 7, 9, 8), (1, 16, 12, 8), (1, 1, 6, 8), (1, 6, 1, 8)]


def close(a, b):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=0, atol=TOL)


def tied(rng, shape):
    """values from {0, 1, 2}: most windows hold several maxima"""
    return rng.integers(0, 3, size=shape).astype(np.float64)


def test_ulp16_is_the_fp16_spacing():
    v = np.array([0.0, 2.0 ** -30, 2.0 ** -24, 2.0 ** -15, 2.0 ** -14, 1.0, 1.5, 2.0, 1000.0, 65504.0])
    want = np.array([2.0 ** -24] * 4 + [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -1, 2.0 ** 5])
    np.testing.assert_array_equal(F.ulp16(v), want)
    np.testing.assert_array_equal(F.ulp16(-v), want)
    h = np.array([2.0 ** -14, 1.0, 1.5, 2.0, 1000.0, 3.0e4], dtype=np.float16)
    np.testing.assert_array_equal(F.ulp16(h), np.spacing(h).astype(np.float64))
    sub = np.array([2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15], dtype=np.float16)
    np.testing.assert_array_equal(F.ulp16(sub), np.spacing(sub).astype(np.float64))
    np.testing.assert_array_equal(F.ulp32(np.array([1.0, 3.0, 0.1])), np.spacing(np.array([1.0, 3.0, 0.1], dtype=np.float32)).astype(np.float64))


def test_cast_is_round_to_nearest_even():
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.9, 65520.0, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 * 1.5], dtype=np.float32)
    want = np.array([1.0, 1.0 + 2.0 ** -9, 65504.0, np.inf, 0.0, 2.0 ** -23, 2.0 ** -23])
    np.testing.assert_array_equal(F.cast_f16(x).astype(np.float64), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_ops_match_the_oracle(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.normal(size=shape)
    n, h, w, c = shape
    if h >= 2 and w >= 2:
        close(F.avgpool2(x), ops.avg_pool2(x))
        close(F.avgpool2(x), R.avg_pool2(R.T(x)).numpy())
    for k, fn in ((2, F.maxpool2), (3, F.maxpool3s2)):
        if k == 3 or (h % 2 == 0 and w % 2 == 0):
            close(fn(x), ops.max_pool(x, k, 2))
            close(fn(x), R.max_pool(R.T(x), k, 2).numpy())
    close(F.resize2x(x), ops.resize_bilinear_2x(x))
    close(F.resize2x(x), R.resize2x(R.T(x)).numpy())
    mh, mw = F._resize_matrix(h), F._resize_matrix(w)
    close(np.einsum("ph,nhwc,qw->npqc", mh, x, mw), ops.resize_bilinear_2x(x))      # the matrices the backward transposes
    close(F.gap(x), ops.global_avg_pool(x))
    mean, var = F.bn_stats(x)
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.normal(size=c)
    close(F.bn_apply(x, mean, var, gamma, beta, 1e-3, False), ops.batch_norm_train(x, gamma, beta)[0])
    p = {"n.gamma": R.T(gamma), "n.beta": R.T(beta)}
    close(F.bn_apply(x, mean, var, gamma, beta, 1e-3, True), torch.relu(R.bn(p, "n", R.T(x), True)).numpy())
    close(mean, x.mean(axis=(0, 1, 2)))
    close(var, x.var(axis=(0, 1, 2)))


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_ops_match_float64_autograd(shape):
    rng = np.random.default_rng(sum(shape) + 1)
    n, h, w, c = shape
    x = rng.normal(size=shape)

    def grad(fn, xin, gy=None):
        t = R.T(xin, True)
        y = fn(t)
        gy = rng.normal(size=tuple(y.shape)) if gy is None else gy
        (y * R.T(gy)).sum().backward()
        return gy, t.grad.numpy()

    if h >= 2 and w >= 2:
        gy, want = grad(R.avg_pool2, x)
        close(F.avgpool2_bwd(gy, shape), want)
    for xin in (x, tied(rng, shape)):
        if h % 2 == 0 and w % 2 == 0:
            gy, want = grad(lambda t: R.max_pool(t, 2, 2), xin)
            close(F.maxpool2_bwd(xin, gy), want)
        gy, want = grad(lambda t: R.max_pool(t, 3, 2), xin)
        close(F.maxpool3s2_bwd(xin, gy), want)
    gy, want = grad(R.resize2x, x)
    close(F.resize2x_bwd(gy, shape), want)
    gy, want = grad(lambda t: t[:, ::2, ::2], x)
    close(F.upsample_zero2(gy, shape), want)
    gy, want = grad(lambda t: t.mean(dim=(1, 2)), x)
    close(F.gap_bwd(gy, shape), want)
    close(F.add(x, 2.0 * x), 3.0 * x)
    close(F.add(x, -2.0 * x, relu=True), np.maximum(-x, 0.0))
    # activations: y = act(z), dz = dy * act'(y)
    for act, fn in ((F.ACT_RELU, torch.relu), (F.ACT_LRELU, R.lrelu), (F.ACT_TANH, torch.tanh), (F.ACT_NONE, lambda t: t * 1.0)):
        t = R.T(x, True)
        y = fn(t)
        gy = rng.normal(size=shape)
        (y * R.T(gy)).sum().backward()
        dz, db = F.act_bwd_bias(gy, y.detach().numpy(), act)
        close(dz, t.grad.numpy())
        close(db, t.grad.numpy().reshape(-1, c).sum(axis=0))
    # BatchNorm (+ relu) with the batch statistics of x
    for relu in (False, True):
        gamma, beta = rng.uniform(0.5, 1.5, c), rng.normal(size=c)
        p = {"n.gamma": R.T(gamma, True), "n.beta": R.T(beta, True)}
        t = R.T(x, True)
        y = R.bn(p, "n", t, True)
        y = torch.relu(y) if relu else y
        gy = rng.normal(size=shape)
        (y * R.T(gy)).sum().backward()
        mean, var = F.bn_stats(x)
        dx, dgamma, dbeta = F.bn_bwd(gy, x, y.detach().numpy() if relu else None, mean, var, gamma, 1e-3)
        close(dx, t.grad.numpy())
        close(dgamma, p["n.gamma"].grad.numpy())
        close(dbeta, p["n.beta"].grad.numpy())
        adx, adg, adb = F.bn_bwd(gy, x, y.detach().numpy() if relu else None, mean, var, gamma, 1e-3, absolute=True)
        assert (adx >= np.abs(dx) - TOL).all() and (adg >= np.abs(dgamma) - TOL).all() and (adb >= np.abs(dbeta) - TOL).all()


@pytest.mark.parametrize("hw", [(2, 2), (2, 3), (5, 7), (7, 9), (16, 12)])
def test_front_end_and_packing_match_the_oracle_and_autograd(hw):
    rng = np.random.default_rng(hw[0] * 31 + hw[1])
    img = np.round(rng.random((2,) + hw + (3,)) * 255.0) / 255.0
    f = F.lin_frontend(img)
    close(f[..., :93], ops.lin_frontend(img))
    assert f.shape[-1] == 96 and not f[..., 93:].any()
    t = R.T(img, True)
    tf = R.lin_frontend(t)
    close(f[..., :93], tf.detach().numpy())
    dF = rng.normal(size=f.shape)
    (tf * R.T(dF[..., :93])).sum().backward()
    close(F.lin_frontend_bwd(img, dF), t.grad.numpy())
    assert (F.lin_frontend_bwd(img, dF, absolute=True) >= np.abs(t.grad.numpy()) - TOL).all()
    assert (F.lin_frontend_abs(img)[..., :93] >= np.abs(f[..., :93]) - TOL).all()
    # packing
    srcs = [rng.random(img.shape) for _ in range(4)]
    for ns, oc in ((1, 8), (2, 8), (3, 16), (4, 16)):
        y = F.pack3(srcs[:ns], oc)
        close(y[..., :3 * ns], np.concatenate(srcs[:ns], -1))
        assert not y[..., 3 * ns:].any()
        for s, o in enumerate(F.unpack3(y, ns)):
            close(o, srcs[s])
    t = R.T(img, True)
    v = R.vgg_preprocess(t)
    close(F.pack3([img], 8, vgg=True)[..., :3], ops.vgg_preprocess(img))
    close(F.pack3([img], 8, vgg=True)[..., :3], v.detach().numpy())
    g = rng.normal(size=img.shape[:-1] + (8,))
    (v * R.T(g[..., :3])).sum().backward()
    close(F.unpack3(g, 1, vgg=True)[0], t.grad.numpy())
    assert (F.pack3_vgg_abs(img) >= np.abs(ops.vgg_preprocess(img))).all()


def test_abs_bound_is_the_op_on_magnitudes():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(2, 5, 7, 8))
    for op, args in (("avgpool2", ()), ("resize2x", ()), ("gap", ()), ("avgpool2_bwd", ((2, 11, 15, 8),)), ("resize2x_bwd", ((2, 2, 3, 8),))):
        if op == "resize2x_bwd":
            xin = rng.normal(size=(2, 4, 6, 8))
        else:
            xin = x
        b = F.abs_bound(op, xin, *args)
        close(b, F._LINEAR[op](np.abs(xin), *args))
        assert (b >= np.abs(F._LINEAR[op](xin, *args)) - TOL).all()
    close(F.abs_bound("add", x, -x), 2 * np.abs(x))
    g = rng.normal(size=(2, 8))
    close(F.abs_bound("gap_bwd", g, (2, 3, 3, 8)), np.broadcast_to(np.abs(g)[:, None, None, :] / 9.0, (2, 3, 3, 8)))
    close(F.abs_bound("upsample_zero2", g.reshape(1, 1, 2, 8), (1, 2, 3, 8))[:, ::2, ::2], np.abs(g).reshape(1, 1, 2, 8))
