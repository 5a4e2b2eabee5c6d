"""tests/tape_replay.py pinned on the CPU: every float64 local reference (forward and VJP) against float64 autograd of the
corresponding tests/torch_ref.py / torch expression at 1e-12, the convolution engine against the independent NumPy statements of
tests/conv_ref.py, and the recorder, the replay, the alias / cut-edge logic and the foreign-node walk on a small torch-only graph
built from stand-in Functions (correct ones pass, each of the three planted errors is reported at exactly its node or variable)."""
import importlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref
import tape_replay as TP
import torch_ref as R
from conftest import rel_err

TOL = 1e-12
SPATIAL = [(1, 1, 1), (1, 2, 2), (1, 2, 3), (2, 5, 7), (1, 7, 9), (1, 16, 12)]      # tests/test_gpu_tape_f32.py
CHANNELS = [4, 12, 20, 64, 132]
EVEN = [(1, 2, 2), (2, 4, 6), (1, 16, 12)]
NHWC = [nhw + (c,) for nhw, c in zip(SPATIAL, CHANNELS + [4])]


def close(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size:
        assert float(np.abs(a - b).max()) <= TOL * max(1.0, float(np.abs(b).max())), (what, float(np.abs(a - b).max()))


def pin(name, args, torch_fn, diff, rng):
    """REFS[name] against float64 autograd of torch_fn at `args` (ndarrays: tensors, anything else: values); diff: differentiable argument
    indices.  The reference's VJP gets torch's outputs as `the device's y`."""
    ref = TP.REFS[name]
    a64 = [np.asarray(a, dtype=np.float64) if isinstance(a, np.ndarray) else a for a in args]
    targs = [R.T(a, i in diff) if isinstance(a, np.ndarray) else a for i, a in enumerate(args)]
    outs = torch_fn(*targs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    want = ref.fwd(*a64)
    assert len(want) == len(outs)
    for w, o in zip(want, outs):
        close(np.asarray(w).reshape(tuple(o.shape)), o.detach().numpy(), name + " forward")
    gs = [rng.normal(size=tuple(o.shape)) for o in outs]
    sum((o * R.T(g)).sum() for o, g in zip(outs, gs)).backward()
    grads = ref.vjp(a64, tuple(o.detach().numpy() for o in outs), tuple(gs))
    assert len(grads) == len(args)
    for i, a in enumerate(args):
        if i in diff:
            close(np.asarray(grads[i]).reshape(a.shape), targs[i].grad.numpy(), "%s grad[%d]" % (name, i))
        else:
            assert grads[i] is None or isinstance(a, np.ndarray), (name, i)
    return grads


def t_act(z, a):
    return {0: z, 1: torch.relu(z), 2: R.lrelu(z), 3: torch.tanh(z)}[a]


# ---- the registry covers the product ----------------------------------------------------------------------------------------------------
def test_every_function_class_of_the_product_has_a_reference():
    A = importlib.import_module("singlehdr-tf2_amd._autograd")
    names = {c.__name__ for c in TP.function_classes(A)}
    assert len(names) >= 29 and names == set(TP.REFS), (sorted(names - set(TP.REFS)), sorted(set(TP.REFS) - names))


def test_bars_are_the_projects_op_level_bars():
    f16, f32 = torch.float16, torch.float32
    assert TP.bar_of("Conv2dFn", "conv", True, f32)[0] == 1e-5 and TP.bar_of("Conv2dFn", "conv", False, f32)[0] == 1e-4
    assert TP.bar_of("BatchNormTrainFn", "bn", True, f32)[0] == 1e-5 and TP.bar_of("BatchNormTrainFn", "bn", False, f32)[0] == 1e-4
    assert TP.bar_of("GapFn", "glue", True, f32)[0] == 1e-5 == TP.bar_of("DiffLossFn", "glue", False, f32)[0]
    assert TP.bar_of("ApplyRfFn", "crf", False, f32)[0] == 2e-4 == TP.bar_of("IncreaseFn", "crf", True, f32)[0]
    assert TP.bar_of("Conv2dHFn", "conv", True, f16)[0] == 2e-3 == TP.bar_of("Conv2dHFn", "conv", True, f32)[0]
    assert TP.bar_of("Conv2dHFn", "conv", False, f16)[0] == 3e-3 == TP.bar_of("Conv2dHFn", "conv", False, f32)[0]
    assert TP.bar_of("AvgPool2Fn", "glue", True, f16)[0] == 2.0 ** -10 == TP.bar_of("BatchNormTrainFn", "bn", False, f16)[0]
    assert TP.bar_of("BatchNormTrainFn", "bn", False, f32)[0] == 1e-4          # dgamma / dbeta of an fp16 node are fp32 results
    # the relative error is conftest.rel_err when no floor applies
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=(3, 4)).astype(np.float32), rng.normal(size=(3, 4))
    e = TP._compare(torch.from_numpy(a), b, idx=0, name="x", item="fwd[0]", shapes=[], plan="", bar=1.0, label="")
    assert e.rel == rel_err(a, b) and e.where == tuple(int(i) for i in np.unravel_index(np.abs(a - b).argmax(), a.shape))


# ---- convolution --------------------------------------------------------------------------------------------------------------------------
CONV = [
    # name, N, H, W, C1, C2, Cout (gemm), k, stride, act, x2_scale, cout_valid
    ("1x1_one_pixel", 1, 1, 1, 4, 0, 4, 1, 1, 0, 1.0, None),
    ("3x3_2x3_lrelu", 1, 2, 3, 12, 0, 20, 3, 1, 2, 1.0, None),
    ("3x3_5x7_relu", 2, 5, 7, 20, 0, 12, 3, 1, 1, 1.0, None),
    ("skip_1x1_x2_scale_255", 2, 5, 7, 16, 16, 8, 1, 1, 0, 1.0 / 255, None),
    ("concat_3x3_x2_scale_half", 1, 7, 9, 8, 12, 16, 3, 1, 1, 0.5, None),
    ("7x7_s2_odd_93_of_96", 2, 7, 9, 96, 0, 8, 7, 2, 1, 1.0, None),
    ("3x3_s2_odd", 1, 7, 9, 4, 0, 8, 3, 2, 2, 1.0, None),
    ("1x1_s2_even", 1, 16, 12, 8, 0, 16, 1, 2, 0, 1.0, None),
    ("7x7_lrelu", 1, 16, 12, 4, 0, 16, 7, 1, 2, 1.0, None),
    ("5x5", 1, 7, 9, 4, 0, 4, 5, 1, 0, 1.0, None),
    ("head_3_of_16_tanh", 2, 5, 7, 16, 0, 16, 3, 1, 3, 1.0, 3),
    ("head_3_of_16_1x1_two_sources", 1, 7, 9, 4, 4, 16, 1, 1, 1, 1.0 / 255, 3),
]


@pytest.mark.parametrize("fn", ["Conv2dFn", "Conv2dHFn"])
@pytest.mark.parametrize("case", CONV, ids=[c[0] for c in CONV])
def test_conv_reference_against_autograd_and_conv_ref(case, fn):
    name, n, h, w, c1, c2, cout, k, stride, a, x2s, cv = case
    rng = np.random.default_rng(len(name) * 7 + h)
    x = rng.normal(size=(n, h, w, c1))
    if c1 == 96:
        x[..., 93:] = 0.0                                    # the front end's padding channels
    x2 = rng.normal(size=(n, h, w, c2)) / x2s if c2 else None
    wt = rng.normal(size=(k, k, c1 + c2, cout)) / np.sqrt(k * k * (c1 + c2))
    ncv = cv or cout
    if cv:
        wt[..., cv:] = 0.0                                   # Conv2D.call_padded pads with zero columns
    b = rng.normal(size=ncv) * 0.1
    s = TP.f32c(x2s)

    def net(tx, tx2, tw, tb, *_):
        xin = tx if tx2 is None else torch.cat([tx, tx2 * s], -1)
        return t_act(R.conv2d(xin, tw[..., :ncv], tb, stride), a)
    tail = (stride, x2s, a, cv) + ((0,) if fn == "Conv2dFn" else ())
    grads = pin(fn, [x, x2, wt, b] + list(tail), net, {0, 2, 3} | ({1} if c2 else set()), rng)
    assert not cv or not grads[2][..., cv:].any()          # nothing in the padded columns
    # the engine against the independent NumPy statements of the forward, the input gradient and the weight gradient
    dz = rng.normal(size=(n, -(-h // stride), -(-w // stride), ncv))
    wv = wt[..., :ncv]
    xin = x if x2 is None else np.concatenate([x, s * x2], -1)
    close(TP.conv_linear(xin, wv, stride), conv_ref.conv2d(x, x2, wv, None, stride, s), "conv_ref.conv2d")
    dxin, dwv = TP.conv_linear_vjp(xin, wv, stride, dz)
    close(dxin[..., :c1], conv_ref.dgrad(dz, wv, x.shape, 0, c1, 1.0, stride), "conv_ref.dgrad")
    if c2:
        close(s * dxin[..., c1:], conv_ref.dgrad(dz, wv, x2.shape, c1, c2, s, stride), "conv_ref.dgrad x2")
    close(dwv, conv_ref.wgrad(x, x2, dz, wv.shape, stride, s, ncv), "conv_ref.wgrad")
    close(dz.reshape(-1, ncv).sum(axis=0), conv_ref.bias_grad(dz), "conv_ref.bias_grad")


def test_conv_reference_without_bias():
    rng = np.random.default_rng(3)
    x, wt = rng.normal(size=(1, 5, 7, 4)), rng.normal(size=(3, 3, 4, 8))
    pin("Conv2dFn", [x, None, wt, None, 1, 1.0, 1, None, 0], lambda tx, _x2, tw, *_: torch.relu(R.conv2d(tx, tw, None, 1)), {0, 2}, rng)


# ---- BatchNorm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 2, 3, 12), (1, 16, 12, 64), (2, 1, 1, 4)], ids=str)
def test_batchnorm_references(shape, relu):
    rng = np.random.default_rng(sum(shape) + relu)
    c = shape[-1]
    x = rng.normal(size=shape) * 2 + 1
    g, b = rng.uniform(0.5, 1.5, c), rng.normal(size=c)
    mm, mv = rng.normal(size=c), rng.uniform(0.5, 2.0, c)
    eps = TP.f32c(1e-3)

    def train(tx, tg, tb, *_):
        y = R.bn({"n.gamma": tg, "n.beta": tb}, "n", tx, True, eps)
        return torch.relu(y) if relu else y
    pin("BatchNormTrainFn", [x, g, b, mm, mv, 1e-3, 0.99, relu], train, {0, 1, 2}, rng)
    res = rng.normal(size=shape)
    for residual, a in ((None, 0), (res, 1 if relu else 0), (None, 1)):
        def frozen(tx, tg, tb, tm, tv, _e, tr, _a):
            y = (tx - tm) / torch.sqrt(tv + eps) * tg + tb
            return t_act(y if tr is None else y + tr, a)
        pin("BatchNormFrozenFn", [x, g, b, mm, mv, 1e-3, residual, a], frozen, {0, 1, 2} | ({6} if residual is not None else set()), rng)
    for scale, shift, residual, a in ((g, b, None, 1), (g, b, res, 1), (None, None, res, 1), (g, None, None, 0), (None, None, None, 3)):
        def aff(tx, ts, th, tr, _a):
            y = tx
            y = y * ts if ts is not None else y
            y = y + th if th is not None else y
            return t_act(y + tr if tr is not None else y, a)
        pin("AffineActFn", [x, scale, shift, residual, a], aff, {0} | ({3} if residual is not None else set()), rng)


# ---- pools, resize, gap, elementwise glue ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", NHWC, ids=str)
def test_simple_family_references(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.normal(size=shape)
    pin("MaxPool3s2Fn", [x], lambda t: R.max_pool(t, 3, 2), {0}, rng)
    pin("Resize2xFn", [x], R.resize2x, {0}, rng)
    pin("GapFn", [x], lambda t: t.mean(dim=(1, 2)), {0}, rng)
    pin("AddFn", [x, rng.normal(size=shape)], lambda a, b: a + b, {0, 1}, rng)
    pin("AddReluFn", [x, rng.normal(size=shape)], lambda a, b: torch.relu(a + b), {0, 1}, rng)
    pin("MarkFn", [x, None], lambda t, _cb: t * 1.0, {0}, rng)
    pin("ForkFn", [x, 3], lambda t, n: tuple(t * 1.0 for _ in range(n)), {0}, rng)
    x3 = rng.random(shape[:3] + (3,)) * 1.4 - 0.2
    pin("ClipFn", [x3, 0.0, 1.0], lambda t, lo, hi: torch.clamp(t, lo, hi), {0}, rng)
    pin("LogcFn", [np.abs(x3)], R.logc, {0}, rng)
    pin("Reverse3Fn", [x3], lambda t: t.flip(-1), {0}, rng)
    for oc in (3, 4, 8, 16):
        pin("VggPreFn", [x3, oc, None], lambda t, o, _d: F.pad(R.vgg_preprocess(t), (0, o - 3)), {0}, rng)
    srcs = [rng.normal(size=shape[:3] + (3,)) for _ in range(3)]
    for oc in (9, 12, 16):
        pin("Pack3Fn", [oc, None] + srcs, lambda o, _d, *ts: F.pad(torch.cat(ts, -1), (0, o - 9)), {2, 3, 4}, rng)
    y12 = rng.normal(size=shape[:3] + (12,))
    for nout in (1, 2, 3):
        pin("Unpack3Fn", [y12, nout], lambda t, k: tuple(t[..., 3 * i:3 * i + 3] for i in range(k)), {0}, rng)


@pytest.mark.parametrize("nhw", EVEN, ids=str)
@pytest.mark.parametrize("c", [4, 12, 132])
def test_two_by_two_pool_references(nhw, c):
    rng = np.random.default_rng(sum(nhw) + c)
    x = rng.normal(size=nhw + (c,))
    pin("AvgPool2Fn", [x], R.avg_pool2, {0}, rng)
    pin("MaxPool2Fn", [x], lambda t: R.max_pool(t, 2, 2), {0}, rng)


def test_fork_reference_skips_unused_aliases():
    g = np.ones((1, 2, 2, 4))
    assert TP.fork_vjp([None, 3], None, (None, None, None)) == (None, None)
    out = TP.fork_vjp([None, 3], None, (g, None, 2 * g))
    assert np.array_equal(out[0], 3 * g) and out[1] is None
    gr = TP.unpack3_vjp([np.zeros((1, 2, 2, 12)), 2], None, (np.ones((1, 2, 2, 3)), None))      # an un-materialised gradient is zero
    assert gr[0].shape == (1, 2, 2, 12) and gr[0][..., :3].all() and not gr[0][..., 3:].any()


# ---- CRF head ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3])
def test_crf_head_references(b, emor_table):
    rng = np.random.default_rng(b)
    feat, wfc, bfc = rng.normal(size=(b, 512)), rng.normal(size=(512, 11)) * 0.05, rng.normal(size=11) * 0.1

    def decode(tf_, tw, tb, tab):
        return tab[:, 0][None] + (tf_ @ tw + tb) @ tab[:, 1:].T
    pin("InvcrfDecodeFn", [feat, wfc, bfc, np.asarray(emor_table, dtype=np.float64)], decode, {0, 1, 2}, rng)
    rf = np.cumsum(rng.random((b, 1024)) - 0.02, axis=1).astype(np.float32).astype(np.float64)      # a few negative slopes: the min is routed
    assert ((rf[:, 1:] - rf[:, :-1]).min(axis=1) < 0).all()
    pin("IncreaseFn", [rf], R.increase, {0}, rng)
    mono = np.cumsum(rng.random((b, 1024)) + 0.01, axis=1)                   # already increasing: no routing
    pin("IncreaseFn", [mono], R.increase, {0}, rng)
    x = (rng.random((b, 5, 7, 3)) * 0.98 + 0.01).astype(np.float32).astype(np.float64)
    lut = np.sort(rng.random((b, 1024)), axis=1)
    pin("ApplyRfFn", [x, lut], R.apply_rf, {0, 1}, rng)


def test_apply_rf_takes_the_knot_from_the_fp32_product():
    """x the largest fp32 number below 5 / 1023: the exact product 1023 x lies below the knot 5, fp32 rounds it onto the knot -- the
    device's floor is 5, and the reference follows it (segment [5, 6], extended linearly below the knot)"""
    x32 = np.float32(5.0 / 1023.0)
    while 1023.0 * float(x32) >= 5.0:
        x32 = np.nextafter(x32, np.float32(0))
    assert np.float32(1023) * x32 == np.float32(5.0) and 1023.0 * float(x32) < 5.0
    x = np.full((1, 1, 1, 1), float(x32))
    lut = (np.arange(1024.0) ** 2)[None] / 1024.0 ** 2
    (y,) = TP.apply_rf_fwd(x, lut)
    dx, drf = TP.apply_rf_vjp([x, lut], (y,), (np.ones_like(x),))
    assert abs(float(y[0, 0, 0, 0]) - lut[0, 5]) < 1e-9 and drf[0, 6] < 0 < drf[0, 5] and not drf[0, 4]
    assert float(dx[0, 0, 0, 0]) == 1023.0 * (lut[0, 6] - lut[0, 5])


def test_increase_takes_its_decisions_from_the_fp32_differences():
    rf = np.array([[0.0, 0.25, 0.25 + 2.0 ** -30, 1.0, 0.5, 2.0]])               # fp32 inputs hold 0.25 twice: slope 0, not 2^-30
    rf32 = rf.astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(0)
    dout = rng.normal(size=rf.shape)
    tr = R.T(rf32, True)
    (R.increase(tr) * R.T(dout)).sum().backward()
    close(TP.increase_bwd(rf32, dout), tr.grad.numpy())


# ---- losses, blends, front end, normalisation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 3), (2, 5, 7, 3), (3, 16, 12, 3)], ids=str)
def test_loss_and_blend_references(shape):
    rng = np.random.default_rng(sum(shape))
    a, b = rng.random(shape), rng.random(shape)
    for mode, fn in ((0, lambda p, q, _m: ((p - q) ** 2).mean(dim=(1, 2, 3))), (1, lambda p, q, _m: (p - q).abs().mean(dim=(1, 2, 3)))):
        pin("DiffLossFn", [a, b, mode], fn, {0, 1}, rng)
    v = rng.random((shape[0], 1024))
    pin("DiffLossFn", [v, rng.random(v.shape), 0], lambda p, q, _m: ((p - q) ** 2).mean(dim=1), {0, 1}, rng)
    pin("TvLossFn", [a], lambda t: R.tv_loss(t).reshape(1), {0}, rng)
    thr = TP.f32c(0.12)
    base = rng.random(shape) * 0.3 + 0.8                      # 0 < alpha < 1, alpha = 0 and alpha = 1 all occur
    hal = rng.normal(size=shape)
    alpha = R.alpha_mask(R.T(base), thr).numpy()
    pin("BlendConstFn", [base, alpha, hal, 0.12], lambda tb, ta, th, _t: tb + ta * th.flip(-1), {2}, rng)
    pin("AlphaBlendFn", [base, hal, 0.12], lambda tb, th, _t: tb + R.alpha_mask(tb, thr) * th.flip(-1), {0, 1}, rng)
    r = rng.random(shape) + 0.1
    e, tg = TP.f32c(1e-6), TP.f32c(0.5)
    pin("MeanNormFn", [r, 1e-6, 0.5], lambda t, _e, _t: t / (e + t.mean(dim=(1, 2, 3), keepdim=True)) * tg, {0}, rng)
    img = rng.random(shape) * 0.98 + 0.01
    if shape[1] > 1:                                           # REFLECT padding needs two rows
        for ch in (93, 96):
            pin("LinFrontendFn", [img, ch, None], lambda t, c, _d: F.pad(R.lin_frontend(t), (0, c - 93)), {0}, rng)


# ---- recorder, replay and structure checks on stand-in Functions ---------------------------------------------------------------------
def standin(fork_drops_last=False, dgrad2_scale=1.0, acc_twice=False):
    """a module of stand-in Functions with the product's class names and argument lists, fp32 torch-CPU arithmetic"""
    M = types.ModuleType("standin")
    M.K = types.SimpleNamespace(PRECISION="fp32")

    class Conv2dFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, x2, w, bias, stride, x2_scale, act1, cout_valid, algo):
            xin = x if x2 is None else torch.cat([x, x2 * x2_scale], -1)
            y = t_act(R.conv2d(xin, w, bias, stride), act1)
            ctx.save_for_backward(x, x2, w, y)
            ctx.meta, ctx.bias_ref = (stride, x2_scale, act1), bias
            return y

        @staticmethod
        def backward(ctx, dy):
            x, x2, w, y = ctx.saved_tensors
            stride, s, a = ctx.meta
            dz = dy * {0: torch.ones_like(y), 1: (y > 0).float(), 2: torch.where(y > 0, 1.0, 0.1), 3: 1 - y * y}[a]
            with torch.enable_grad():
                xin = (x if x2 is None else torch.cat([x, x2 * s], -1)).detach().requires_grad_(True)
                wd = w.detach().requires_grad_(True)
                gx, gw = torch.autograd.grad(R.conv2d(xin, wd, None, stride), [xin, wd], dz)
            c1 = x.shape[3]
            db = dz.sum(dim=(0, 1, 2)) if ctx.bias_ref is not None else None
            if getattr(w, "_acc", False):                      # the `_acc` fast path: add into the gradient buffer, return None
                for _ in range(2 if acc_twice else 1):
                    w.grad += gw
                gw = None
            dx2 = None if x2 is None else gx[..., c1:] * s * dgrad2_scale
            return (gx[..., :c1] if ctx.needs_input_grad[0] else None), dx2, gw, db, None, None, None, None, None

    class ForkFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, n):
            ctx.set_materialize_grads(False)
            return tuple(x.view_as(x) for _ in range(n))

        @staticmethod
        def backward(ctx, *gs):
            if fork_drops_last:
                gs = gs[:-1]
            gs = [g for g in gs if g is not None]
            return (sum(gs[1:], gs[0]) if gs else None), None

    class MarkFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, callback):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, g):
            return g, None

    class ClipFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, lo, hi):
            ctx.save_for_backward(x)
            ctx.meta = (lo, hi)
            return x.clamp(lo, hi)

        @staticmethod
        def backward(ctx, dy):
            (x,) = ctx.saved_tensors
            return dy * ((x >= ctx.meta[0]) & (x <= ctx.meta[1])), None, None

    class DiffLossFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b, mode):
            ctx.save_for_backward(a, b)
            return ((a - b) ** 2).mean(dim=(1, 2, 3))

        @staticmethod
        def backward(ctx, g):
            a, b = ctx.saved_tensors
            d = 2 * (a - b) * g.reshape(-1, 1, 1, 1) / a[0].numel()
            return (d if ctx.needs_input_grad[0] else None), (-d if ctx.needs_input_grad[1] else None), None

    for c in (Conv2dFn, ForkFn, MarkFn, ClipFn, DiffLossFn):
        setattr(M, c.__name__, c)
    return M


def run_standin(M, acc=True):
    """conv(3 -> 8, lrelu) -> fork -> [conv(8 + 8 skip, padded 3-of-16 head, shared nothing), mark] -> clip -> loss * mask, sum; the
    first filter sits in a gradient buffer (`_acc`), the head filter is a zero-padded view of its variable"""
    g = torch.Generator().manual_seed(0)
    x = torch.rand((2, 6, 5, 3), generator=g)
    tgt = torch.rand((2, 6, 5, 3), generator=g)
    w1 = (torch.randn((3, 3, 3, 8), generator=g) * 0.3).requires_grad_(True)
    b1 = (torch.randn(8, generator=g) * 0.1).requires_grad_(True)
    w2 = (torch.randn((1, 1, 16, 3), generator=g) * 0.3).requires_grad_(True)
    b2 = (torch.randn(3, generator=g) * 0.1 + 0.5).requires_grad_(True)
    if acc:
        w1.grad = torch.zeros_like(w1)
        w1._acc = True
    variables = [("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)]
    with TP.record(M) as rec:
        t = M.Conv2dFn.apply(x, None, w1, b1, 1, 1.0, 2, None, 0)
        skip, main, unused = M.ForkFn.apply(t, 3)
        main = M.MarkFn.apply(main, None)
        y = M.Conv2dFn.apply(main, skip, w2, b2, 1, 0.5, 0, None, 0)
        loss = M.DiffLossFn.apply(M.ClipFn.apply(y, 0.0, 1.0), tgt, 0) * torch.tensor([1.0, 0.5])
        loss.sum().backward()
    return rec, variables, dict(x=x, t=t, y=y)


def test_recorder_stores_calls_in_tape_order_with_node_level_gradients():
    M = standin()
    rec, variables, _ = run_standin(M)
    assert [n.name for n in rec.nodes] == ["Conv2dFn", "ForkFn", "MarkFn", "Conv2dFn", "ClipFn", "DiffLossFn"]
    assert [n.idx for n in rec.nodes] == list(range(6)) and all(n.prec == "fp32" for n in rec.nodes)
    assert "apply" not in vars(M.Conv2dFn) and len(rec.roots) == 1                      # `.apply` is restored
    c1, fork, _, c2, clip, loss = rec.nodes
    assert c1.args[2] is variables[0][1] and c1.args[4:] == [1, 1.0, 2, None, 0] and c1.single and not fork.single
    assert all(n.hook_calls == 1 for n in rec.nodes)
    # gradients per NODE, aligned with the arguments; the `_acc` filter and the data input get None
    assert len(c1.grad_inputs) == 3                                                   # one per tensor argument: x, w, bias
    g1 = c1.aligned_grad_inputs()
    assert len(g1) == 9 and g1[0] is None and g1[2] is None and g1[3] is not None and g1[1] is None
    assert len(fork.grad_outputs) == 3 and fork.grad_outputs[2] is None                # the unused alias
    assert torch.equal(fork.grad_inputs[0], fork.grad_outputs[0] + fork.grad_outputs[1])
    assert torch.equal(c2.aligned_grad_inputs()[1], fork.grad_outputs[0])                         # the skip's own gradient, not a sum
    assert loss.aligned_grad_inputs()[1] is None and tuple(loss.grad_outputs[0].shape) == (2,)


def test_replay_passes_on_correct_standins_and_sums_per_variable():
    M = standin()
    rec, variables, _ = run_standin(M)
    rep = TP.replay(rec, variables)
    rep.assert_ok()
    assert len(rep.entries) == (1 + 3 + 1 + 1 + 1 + 1) + (1 + 1 + 1 + 4 + 1 + 1) and len(rep.var_entries) == 4     # forwards + gradients
    assert not rep.unconsumed and not rep.no_grad and rep.other_leaves == 0
    assert rep.closest(2).count("of its bar") == 2 and "Conv2dFn" in rep.summary() and rep.text().count("\n") + 1 == len(rep.entries) + 4
    # a variable nobody consumes, and one that ends without a gradient, are reported
    lonely = torch.zeros(3, requires_grad=True)
    rep = TP.replay(rec, variables + [("lonely", lonely)])
    assert rep.unconsumed == ["lonely"]
    with pytest.raises(AssertionError):
        rep.assert_ok()
    variables[1][1].grad = None
    assert TP.replay(rec, variables).no_grad == ["b1"]


def test_replay_follows_a_padded_filter_back_to_its_variable_and_sums_shared_weights():
    M = standin()
    g = torch.Generator().manual_seed(1)
    x = torch.rand((1, 5, 4, 4), generator=g)
    w = (torch.randn((3, 3, 4, 3), generator=g) * 0.3).requires_grad_(True)
    wp = F.pad(w, (0, 5, 0, 0))
    with TP.record(M) as rec:
        y1 = M.Conv2dFn.apply(x, None, wp, None, 1, 1.0, 1, None, 0)
        y2 = M.Conv2dFn.apply(x * 0.5, None, w, None, 1, 1.0, 0, None, 0)
        (y1.sum() + (y2 * y2).sum()).backward()
    assert TP.variable_of(wp) is w and TP.variable_of(w) is w and TP.variable_of(x) is None and TP.variable_of(y1) is None
    rep = TP.replay(rec, [("w", w)])
    rep.assert_ok()
    (e,) = rep.var_entries
    assert e.plan.startswith("sum of 2 node(s): #0,#1") and e.shapes == [(3, 3, 4, 3)]
    assert TP.foreign_nodes(rec) == {"AddBackward0": 1, "SumBackward0": 2, "MulBackward0": 1, "ConstantPadNdBackward0": 1, "AccumulateGrad": 1}


def test_replay_reports_exactly_the_planted_errors():
    rec, variables, _ = run_standin(standin())
    fork = rec.of("ForkFn")[0].idx
    conv2 = rec.of("Conv2dFn")[1].idx
    # a ForkFn that drops its last live gradient: only that node, no variable (the nodes behind it are fed the device's own gradient)
    rec, variables, _ = run_standin(standin(fork_drops_last=True))
    assert rec.of("ForkFn")[0].grad_outputs[2] is None                     # the last alias is unused here: dropping it changes nothing
    TP.replay(rec, variables).assert_ok()
    M = standin(fork_drops_last=True)
    g = torch.Generator().manual_seed(2)
    x = torch.rand((1, 4, 4, 3), generator=g).requires_grad_(True)
    with TP.record(M) as rec2:
        a, b = M.ForkFn.apply(M.ClipFn.apply(x, 0.0, 1.0), 2)
        (M.ClipFn.apply(a, 0.2, 0.8) * 2.0 + M.ClipFn.apply(b, 0.1, 0.9)).sum().backward()
    assert TP.replay(rec2).failed_items() == ({(1, "grad[0]")}, set())
    # dx2 of the second source scaled by 1 + 1e-3: only grad[1] of the two-source node
    rec, variables, _ = run_standin(standin(dgrad2_scale=1.0 + 1e-3))
    rep = TP.replay(rec, variables)
    assert rep.failed_items() == ({(conv2, "grad[1]")}, set()), rep.text(True)
    with pytest.raises(AssertionError, match="grad\\[1\\]"):
        rep.assert_ok()
    rep.assert_ok(leave=lambda e: e.idx == conv2 and e.item == "grad[1]")        # left to another assertion: everything else is inside
    with pytest.raises(AssertionError, match="grad\\[1\\]"):
        rep.assert_ok(leave=lambda e: e.item == "grad[0]")
    # a weight gradient accumulated twice through the `_acc` path: only that variable
    rec, variables, _ = run_standin(standin(acc_twice=True))
    assert TP.replay(rec, variables).failed_items() == (set(), {"w1"})
    assert fork == 1


def test_unknown_function_class_raises():
    M = standin()

    class LaterFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2.0

        @staticmethod
        def backward(ctx, g):
            return g * 2.0
    M.LaterFn = LaterFn                                        # a class added to the module later is found by introspection ...
    assert LaterFn in TP.function_classes(M)
    x = torch.rand((1, 2, 2, 3), requires_grad=True)
    with TP.record(M) as rec:
        M.LaterFn.apply(M.ClipFn.apply(x, 0.0, 1.0)).sum().backward()
    assert [n.name for n in rec.nodes] == ["ClipFn", "LaterFn"]
    with pytest.raises(KeyError, match="LaterFn"):              # ... and replayed or refused, never skipped
        TP.replay(rec)


def test_cut_edges_aliases_and_foreign_nodes():
    M = standin()
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 4, 4, 3), generator=g).requires_grad_(True)
    data = torch.rand((2, 4, 4, 3), generator=g)
    with TP.record(M) as rec:
        c = M.ClipFn.apply(x, 0.1, 0.9)                                     # 0
        a, b = M.ForkFn.apply(c, 2)                                         # 1
        m = M.MarkFn.apply(b, None)                                         # 2
        l1 = M.DiffLossFn.apply(a, c.detach(), 0)                           # 3: the same storage as #0's output, arriving constant
        l2 = M.DiffLossFn.apply(m, b.detach(), 0)                           # 4: a detached Fork alias: the storage of #0's output again
        l3 = M.DiffLossFn.apply(torch.relu(m) * 1.0, data, 0)               # 5: torch arithmetic in the middle; `data` has no producer
        with torch.no_grad():
            const = M.ClipFn.apply(data, 0.0, 0.5)                          # 6: an output that never required grad
        l4 = M.DiffLossFn.apply(m, const, 0)                                # 7: no cut
        (l1 + l2 + l3 + l4).sum().backward()
    assert TP.cut_edges(rec) == [("ClipFn", 0, "DiffLossFn", 1), ("ClipFn", 0, "DiffLossFn", 1)]
    assert [n.idx for n in rec.nodes if n.name == "DiffLossFn"] == [3, 4, 5, 7]
    found = TP.foreign_nodes(rec)
    assert found == {"AddBackward0": 3, "SumBackward0": 1, "ReluBackward0": 1, "MulBackward0": 1, "AccumulateGrad": 1}
    assert TP.foreign_nodes(rec, roots=[l1]) == {"AccumulateGrad": 1}
    assert [id(t) for t in TP.reached_variables(rec)] == [id(x)]
    # the Mark output is handed to three consumers as one object: autograd's own add sums them
    assert TP.unforked_fanouts(rec) == [("MarkFn", ("DiffLossFn", "DiffLossFn"))]
    TP.replay(rec).assert_ok()
