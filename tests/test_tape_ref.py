"""tests/tape_ref.py (the float64 reference of the fp32 tape ops, used by tests/test_gpu_tape_f32.py) pinned at 1e-12 to oracle/ops.py,
tests/torch_ref.py and float64 autograd.  The definitions it shares with tests/fp16_ref.py are pinned by tests/test_fp16_ref.py."""
import numpy as np
import pytest
import torch

import fp16_ref
import tape_ref as F
import torch_ref as R
from oracle import ops

TOL = 1e-12


def close(a, b, tol=TOL):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=0, atol=tol)


def grad_of(fn, *xs, gy=None, rng=None):
    """(gy, grads) of sum(fn(*xs) * gy) in float64 autograd"""
    ts = [R.T(x, True) for x in xs]
    y = fn(*ts)
    gy = rng.normal(size=tuple(y.shape)) if gy is None else gy
    (y * R.T(gy)).sum().backward()
    return gy, [t.grad.numpy() for t in ts]


def test_shared_definitions_are_the_fp16_reference_ones():
    for name in ("avgpool2", "avgpool2_bwd", "maxpool2_bwd", "maxpool3s2_bwd", "resize2x", "resize2x_bwd", "upsample_zero2", "gap", "gap_bwd",
                 "bn_stats", "bn_apply", "bn_bwd", "act_grad", "act_bwd_bias", "add", "pack3", "unpack3", "pad_channels", "lin_frontend_bwd", "ulp32"):
        assert getattr(F, name) is getattr(fp16_ref, name), name


def test_bars():
    assert F.bar32(3, -2.0) == 6 * 2.0 ** -24
    t = np.array([[1.0, -2.0, 3.0], [0.5, 0.5, -1.0]])
    close(F.sum_bar(t, axis=1), 2 * 2.0 ** -24 * np.array([6.0, 2.0]))
    close(F.sum_bar(t, extra=2), 7 * 2.0 ** -24 * 8.0)
    # it does bound an fp32 sum, in forward and in pairwise order
    rng = np.random.default_rng(0)
    v = rng.normal(size=4096).astype(np.float32)
    seq = np.float32(0)
    for e in v:
        seq = np.float32(seq + e)
    exact = v.astype(np.float64).sum()
    assert abs(float(seq) - exact) <= F.sum_bar(v) and abs(float(v.sum()) - exact) <= F.sum_bar(v)


@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (2, 5, 7, 3), (1, 16, 12, 3)])
def test_glue_ops_match_the_oracle_and_autograd(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.random(shape) * 1.4 - 0.2
    x.reshape(-1)[:2] = (0.0, 1.0)                                 # the closed ends of the interval
    close(F.clip(x, 0.0, 1.0), np.clip(x, 0.0, 1.0))
    gy, (want,) = grad_of(lambda t: torch.clamp(t, 0.0, 1.0), x, rng=rng)
    close(F.clip_bwd(gy, x, 0.0, 1.0), want)                       # torch passes the gradient on the closed interval too
    assert F.clip_bwd(np.ones(2), np.array([0.0, 1.0]), 0.0, 1.0).tolist() == [1.0, 1.0]
    xp = np.abs(x)
    close(F.logc(xp), ops.log_compress(xp))
    gy, (want,) = grad_of(R.logc, xp, rng=rng)
    close(F.logc_bwd(gy, xp), want)
    close(F.reverse3(x), ops.reverse_channels(x))
    close(F.vgg_preprocess(x, 3), ops.vgg_preprocess(x))
    v4 = F.vgg_preprocess(x, 4)
    close(v4[..., :3], ops.vgg_preprocess(x))
    assert v4.shape[-1] == 4 and not v4[..., 3].any()
    gy, (want,) = grad_of(R.vgg_preprocess, x, rng=rng)
    close(F.vgg_preprocess_bwd(gy), want)
    close(F.vgg_preprocess_bwd(np.concatenate([gy, rng.normal(size=shape[:-1] + (1,))], -1)), want)
    # alpha mask / blend
    b = rng.random(shape) * 0.3 + 0.8
    hal = rng.normal(size=shape)
    close(np.tile(F.alpha_mask(b, 0.12), (1, 1, 1, 3)), ops.alpha_mask(b, 0.12))
    close(F.alpha_mask(b, 0.12), R.alpha_mask(R.T(b), 0.12).numpy())
    a, al = F.alpha_blend(b, hal, 0.12)
    close(a, ops.alpha_blend(b, hal, 0.12))
    close(al, F.alpha_mask(b, 0.12))
    gy, (want,) = grad_of(lambda h: R.T(b) + R.T(al) * h.flip(-1), hal, rng=rng)
    close(F.alpha_blend_bwd(gy, al), want)
    gy, (wb, wh) = grad_of(lambda bb, h: bb + R.alpha_mask(bb, 0.12) * h.flip(-1), b, hal, rng=rng)
    dB, dhal = F.alpha_blend_full_bwd(b, hal, gy, 0.12)
    close(dB, wb)
    close(dhal, wh)


@pytest.mark.parametrize("a", [F.ACT_NONE, F.ACT_RELU, F.ACT_LRELU, F.ACT_TANH])
def test_affine_act(a):
    rng = np.random.default_rng(a)
    x, res = rng.normal(size=(2, 3, 5, 12)), rng.normal(size=(2, 3, 5, 12))
    sc, sh = rng.normal(size=12), rng.normal(size=12)
    fn = {F.ACT_NONE: lambda t: t, F.ACT_RELU: torch.relu, F.ACT_LRELU: R.lrelu, F.ACT_TANH: torch.tanh}[a]
    for use in range(8):
        s, t, r = (sc if use & 1 else None), (sh if use & 2 else None), (res if use & 4 else None)
        want = R.T(x) * (R.T(s) if s is not None else 1.0) + (R.T(t) if t is not None else 0.0) + (R.T(r) if r is not None else 0.0)
        close(F.affine_act(x, s, t, r, a), fn(want).numpy())
        assert (F.affine_pre(x, s, t, r, absolute=True) >= np.abs(F.affine_pre(x, s, t, r)) - TOL).all()
    close(F.act(x, F.ACT_LRELU), ops.leaky_relu(x))
    bn = ops.batch_norm_infer(x, sc, sh, sh, np.abs(sc) + 0.5)     # the folded BatchNorm the op replaces
    inv = sc / np.sqrt(np.abs(sc) + 0.5 + 1e-3)
    close(F.affine_act(x, inv, sh - sh * inv), bn)


@pytest.mark.parametrize("b,f", [(1, 1), (3, 37)])
def test_invcrf_decode_and_bwd(b, f, emor_table):
    rng = np.random.default_rng(b + f)
    table = emor_table.astype(np.float64)
    feat, wfc, bfc = rng.normal(size=(b, f)), rng.normal(size=(f, 11)) * 0.1, rng.normal(size=11)
    want = ops.invcrf_pca_decode(ops.dense(feat, wfc, bfc), table[:, 0], table[:, 1:12])
    close(F.invcrf_decode(feat, wfc, bfc, table), want)
    tab = R.T(table)
    gy, (wf, ww, wb) = grad_of(lambda x, w, bb: tab[:, 0][None, :] + (x @ w + bb) @ tab[:, 1:12].T, feat, wfc, bfc, rng=rng)
    dfeat, dwfc, dbfc = F.invcrf_decode_bwd(gy, feat, wfc, table)
    close(dfeat, wf)
    close(dwfc, ww)
    close(dbfc, wb)
    for got, ref in zip(F.invcrf_decode_bwd(gy, feat, wfc, table, absolute=True), (dfeat, dwfc, dbfc)):
        assert (got >= np.abs(ref) - TOL).all()


def increase_rows(rng, k):
    """monotone; one negative step in the middle; the minimum at the first gap; at the last gap"""
    rows = []
    for kind in range(4):
        g = rng.random(k - 1) + 0.05
        if kind and k > 2:                  # (K = 2 has one gap: a negative one shifts to a zero sum, 0 / 0)
            g[{1: (k - 1) // 2, 2: 0, 3: k - 2}[kind]] = -0.5
        rows.append(np.concatenate([[0.0], np.cumsum(g)]))
    return np.stack(rows)


@pytest.mark.parametrize("k", [2, 3, 257, 1024])
def test_increase_and_bwd(k):
    rng = np.random.default_rng(k)
    rf = increase_rows(rng, k)
    close(F.increase(rf), ops.increase(rf))
    close(F.increase(rf), R.increase(R.T(rf)).numpy())
    gy, (want,) = grad_of(R.increase, rf, rng=rng)
    close(F.increase_bwd(rf, gy), want)


@pytest.mark.parametrize("k", [2, 1024])
def test_apply_rf_and_bwd(k):
    rng = np.random.default_rng(k)
    x = rng.random((3, 4, 5, 3))
    x.reshape(-1)[:4] = (0.0, 1.0, 1.0 / (k - 1), 0.5)
    rf = np.sort(rng.random((3, k)), axis=1)
    close(F.apply_rf(x, rf), ops.apply_rf(x, rf))
    yv, i0, i1, w0, w1 = F.apply_rf_parts(x, k)
    close((w0 * np.take_along_axis(rf, i0, 1) + w1 * np.take_along_axis(rf, i1, 1)).reshape(x.shape), ops.apply_rf(x, rf))
    xi = rng.random((3, 4, 5, 3)) * 0.98 + 0.01                     # off the knots: differentiable in x
    gy, (wx, wr) = grad_of(R.apply_rf, xi, rf, rng=rng)
    drf, dx = F.apply_rf_bwd(xi, rf, gy)
    close(drf, wr)
    close(dx, wx)
    adrf, adx = F.apply_rf_bwd(xi, rf, gy, absolute=True)
    assert (adrf >= np.abs(drf) - TOL).all() and (adx >= np.abs(dx) - TOL).all()


@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (3, 5, 7, 3), (2, 1, 6, 3), (2, 6, 1, 4)])
def test_losses_match_the_oracle_and_autograd(shape):
    rng = np.random.default_rng(sum(shape))
    a, b = rng.normal(size=shape), rng.normal(size=shape)
    close(F.diff_loss(a, b, 0), ops.l2_loss_with_mask(a, b).reshape(-1))
    close(F.diff_loss(a, b, 1), ops.l1_loss_per_sample(a, b).reshape(-1))
    g = rng.normal(size=shape[0])
    da0 = rng.normal(size=shape)
    for mode, fn in ((0, lambda t: ((t - R.T(b)) ** 2).mean(dim=(1, 2, 3))), (1, lambda t: (t - R.T(b)).abs().mean(dim=(1, 2, 3)))):
        _, (want,) = grad_of(fn, a, gy=g)
        close(F.diff_loss_bwd(a, b, g, mode), want)
        close(F.diff_loss_bwd(a, b, g, mode, da0), da0 + want)
    close(F.tv_loss(a), ops.tv_loss(a))
    close(F.tv_loss(a), R.tv_loss(R.T(a)).numpy())
    _, (want,) = grad_of(R.tv_loss, a, gy=np.asarray(0.7))
    close(F.tv_loss_bwd(a, [0.7]), want)
    close(F.tv_loss_bwd(a, [0.7], da0), da0 + want)
    assert np.abs(F.tv_sign_sum(a)).max() <= 4
    # per-sample sums and the mean normalisation
    close(F.sample_dot(a), a.reshape(shape[0], -1).sum(axis=1))
    close(F.sample_dot(a, b), (a * b).reshape(shape[0], -1).sum(axis=1))
    r = np.abs(a) + 0.1
    norm = lambda t: t / (1e-6 + t.mean(dim=(1, 2, 3), keepdim=True)) * 0.5
    close(F.mean_norm_fwd(r, F.sample_dot(r), 1e-6, 0.5), norm(R.T(r)).numpy())
    gy, (want,) = grad_of(norm, r, rng=rng)
    close(F.mean_norm_bwd(gy, F.sample_dot(r), F.sample_dot(gy, r), 1e-6, 0.5), want)
    assert (F.mean_norm_bwd(gy, F.sample_dot(r), F.sample_dot(gy, r), 1e-6, 0.5, absolute=True) >= np.abs(want) - TOL).all()


@pytest.mark.parametrize("B", [4, 5, 16])
def test_soft_hist_and_bwd(B):
    rng = np.random.default_rng(B)
    img = np.round(rng.random((2, 5, 7, 3)) * 255.0) / 255.0
    close(F.soft_hist(img, B), ops.histogram_layer(img, B))

    def hist(t):
        outs = []
        for i in range(1, B + 1):
            d = (t - (2.0 * i - 1.0) / (2.0 * B)).abs()
            outs.append(torch.where(d < 1.0 / B, 1.0 - d * B, torch.zeros_like(d)))
        return torch.cat(outs, -1)
    gy, (want,) = grad_of(hist, img, rng=rng)
    close(F.soft_hist_bwd(img, gy, B), want)
    assert (F.soft_hist_bwd(img, gy, B, absolute=True) >= np.abs(want) - TOL).all()


@pytest.mark.parametrize("gs", [1.0, 2.0 ** -7])
def test_adam_is_the_keras_formula(gs):
    """two steps against torch.optim.Adam restated in Keras form: eps outside the root, no amsgrad, bias correction folded into lr_t"""
    rng = np.random.default_rng(3)
    p, m, v = rng.normal(size=50), np.zeros(50), np.zeros(50)
    b1, b2, eps, lr = 0.9, 0.999, 1e-7, 1e-3
    pk, mk, vk = p.copy(), m.copy(), v.copy()
    for t in (1, 2):
        g = rng.normal(size=50)
        lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        p, m, v = F.adam(p, g / gs, m, v, lr_t, b1, b2, eps, gs)
        mk = b1 * mk + (1 - b1) * g
        vk = b2 * vk + (1 - b2) * g ** 2
        pk = pk - lr_t * mk / (np.sqrt(vk) + eps)
        close(p, pk)
        close(m, mk)
        close(v, vk)
    # and it agrees with torch's Adam up to where eps sits (torch: sqrt(v_hat) + eps): eps -> 0 makes the two the same update
    tp = torch.tensor(pk * 0 + 1.0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=1e-30)
    tp.grad = torch.ones_like(tp) * 0.25
    opt.step()
    q, _, _ = F.adam(np.ones(50), np.full(50, 0.25), np.zeros(50), np.zeros(50), lr * np.sqrt(1.0 - b2) / (1.0 - b1), b1, b2, 1e-30)
    close(q, tp.detach().numpy())
