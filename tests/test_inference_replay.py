"""tests/inference_replay.py pinned on the CPU: the glue references (inference epilogue, `cout_valid`, pooled / projected outputs, the
bilinear prologue) against oracle.nets' own float64 layers at 1e-12, the derived-operand formulas and their counted bars on CPU models
(the planted fold error is caught at exactly the folded shifts and what is built from them), and the recorder's bookkeeping -- nesting,
snapshots, tuple / None returns, the closed-chain check with a planted gap, the C ABI names, the range audit -- on a stub module."""
import importlib
import types

import numpy as np
import pytest
import torch

import inference_replay as IR
import tape_replay as TP
from oracle import nets, ops

TOL = 1e-12
RELU, LRELU, TANH = 1, 2, 3


def close(a, b, what=""):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float(np.abs(a - b).max()) <= TOL * max(1.0, float(np.abs(b).max())), (what, float(np.abs(a - b).max()))


def pad(a, axis, n):
    shape = list(a.shape)
    shape[axis] = n - a.shape[axis]
    return np.concatenate([a, np.zeros(shape)], axis=axis)


def conv_operands(**kw):
    a = dict(x=None, w=None, bias=None, stride=1, x2=None, x2_scale=1.0, act1=0, scale=None, shift=None, residual=None, act2=0, algo=0,
             out=None, cout_valid=None, pad=None, out_hw=None, w_batch_stride=0)
    a.update(kw)
    return a


# ---- 1. the glue against the oracle's own layers -------------------------------------------------------------------------------------
def test_unet_launch_forms_equal_the_oracles_layers():
    """the launches of the Dequantization- / Refinement-Net: padded 3 -> 4 stem, conv + average pool, the bilinear prologue, the
    two-source layer, and the two `cout_valid` heads (tanh + residual; residual with a channel stride + relu)"""
    rng = np.random.default_rng(0)
    p = {k: v.astype(np.float64) for k, v in nets.init_params(nets.deq_spec(), 5).items()}
    x = rng.random((2, 8, 12, 3))
    lr, c = ops.leaky_relu, lambda name, t: ops.conv2d(t, p[name + ".kernel"], p[name + ".bias"])      # noqa: E731
    t = lr(c("conv1", x))
    close(IR._conv2d(conv_operands(x=pad(x, 3, 4), w=pad(p["conv1.kernel"], 2, 4), bias=p["conv1.bias"], act1=LRELU, cout_valid=16))[0], t, "stem")
    s1 = lr(c("conv2", t))
    y, yp = IR._conv2d_avgpool2(dict(x=t, w=p["conv2.kernel"], bias=p["conv2.bias"], act1=LRELU, x2=None))
    close(y, s1, "conv + avgpool: y")
    close(yp, ops.avg_pool2(s1), "conv + avgpool: pooled")
    low = rng.normal(size=(2, 3, 5, 32))
    u = lr(c("u1.conv1", ops.resize_bilinear_2x(low)))
    (got,) = IR._conv2d_up2(dict(x=low, w=p["u1.conv1.kernel"], bias=p["u1.conv1.bias"], act1=LRELU, scale=None, shift=None, act2=0, proj=None))
    close(got, u, "bilinear prologue")
    skip = rng.normal(size=u.shape)
    close(IR._conv2d(conv_operands(x=u, x2=skip, w=p["u1.conv2.kernel"], bias=p["u1.conv2.bias"], act1=LRELU))[0],
          lr(c("u1.conv2", np.concatenate([u, skip], axis=-1))), "two sources")
    f = rng.normal(size=(2, 8, 12, 16))
    w16 = pad(p["out.kernel"], 3, 16)
    close(IR._conv2d(conv_operands(x=f, w=w16, bias=p["out.bias"], act1=TANH, residual=x, cout_valid=3))[0], x + np.tanh(c("out", f)), "deq head")
    x12 = np.concatenate([x, rng.random((2, 8, 12, 6)), np.zeros((2, 8, 12, 3))], axis=-1)
    close(IR._conv2d(conv_operands(x=f, w=w16, bias=p["out.bias"], residual=x12, act2=RELU, cout_valid=3))[0],
          ops.relu(x12[..., :3] + c("out", f)), "ref head")


def bn_of(p, name):
    return types.SimpleNamespace(gamma=torch.from_numpy(p[name + ".gamma"]), beta=torch.from_numpy(p[name + ".beta"]),
                                 moving_mean=torch.from_numpy(p[name + ".moving_mean"]), moving_variance=torch.from_numpy(p[name + ".moving_variance"]))


def test_linearization_launch_forms_equal_the_oracles_layers():
    """conv -> folded BatchNorm -> + residual -> relu in ONE launch, strided and with the zero-padded stem"""
    rng = np.random.default_rng(1)
    p = {k: v.astype(np.float64) for k, v in nets.init_params(nets.lin_spec(), 6).items()}
    q = "crf_feature_net."
    bn = lambda name, t: ops.batch_norm_infer(t, *(p[name + s] for s in (".gamma", ".beta", ".moving_mean", ".moving_variance")))   # noqa: E731
    x = rng.normal(size=(2, 9, 10, 93))
    sc, sh, _ = IR.folded_formula(bn_of(p, q + "norm1"))
    close(IR._conv2d(conv_operands(x=pad(x, 3, 96), w=pad(p[q + "conv1.kernel"], 2, 96), bias=p[q + "conv1.bias"], stride=2, scale=sc, shift=sh,
                                   act2=RELU, cout_valid=64))[0],
          ops.relu(bn(q + "norm1", ops.conv2d(x, p[q + "conv1.kernel"], p[q + "conv1.bias"], 2))), "stem")
    t = rng.normal(size=(2, 5, 6, 256))
    n1 = rng.normal(size=(2, 3, 3, 512))
    a = rng.normal(size=(2, 3, 3, 128))
    sc, sh, _ = IR.folded_formula(bn_of(p, q + "res4.norm4"))
    close(IR._conv2d(conv_operands(x=a, w=p[q + "res4.conv4.kernel"], scale=sc, shift=sh, residual=n1, act2=RELU))[0],
          ops.relu(n1 + bn(q + "res4.norm4", ops.conv2d(a, p[q + "res4.conv4.kernel"]))), "res join")
    sc, sh, _ = IR.folded_formula(bn_of(p, q + "res4.norm1"))
    close(IR._conv2d(conv_operands(x=t, w=p[q + "res4.conv1.kernel"], stride=2, scale=sc, shift=sh))[0],
          bn(q + "res4.norm1", ops.conv2d(t, p[q + "res4.conv1.kernel"], None, 2)), "strided 1x1 shortcut")


@pytest.fixture(scope="module")
def hal_small():
    """the Hallucination-Net's first and last level at 8 x 12: parameters of those layers only"""
    spec = [e for e in nets.hal_spec() if e[0].split(".")[0] in ("u1", "s1", "conv2", "norm2", "d1")]
    return {k: v.astype(np.float64) for k, v in nets.init_params(spec, 7).items()}


def test_hallucination_launch_forms_equal_the_oracles_layers(hal_small):
    p = hal_small
    rng = np.random.default_rng(2)
    bn = lambda name, t: ops.batch_norm_infer(t, *(p[name + s] for s in (".gamma", ".beta", ".moving_mean", ".moving_variance")))   # noqa: E731
    f = rng.normal(size=(2, 8, 12, 64))
    y = ops.relu(ops.conv2d(f, p["d1.conv2.kernel"], p["d1.conv2.bias"]))
    got = IR._conv2d_maxpool2(dict(x=f, w=p["d1.conv2.kernel"], bias=p["d1.conv2.bias"], act1=RELU, keep_y=True, proj=None))
    close(got[0], y, "conv + maxpool: y")
    close(got[1], ops.max_pool(y, 2, 2), "conv + maxpool: pooled")
    (only,) = IR._conv2d_maxpool2(dict(x=f, w=p["d1.conv2.kernel"], bias=p["d1.conv2.bias"], act1=RELU, keep_y=False, proj=None))
    close(only, ops.max_pool(y, 2, 2), "pooled alone")
    low = rng.normal(size=(2, 4, 6, 128))
    up = ops.relu(bn("u1.norm1", ops.relu(ops.conv2d(ops.resize_bilinear_2x(low), p["u1.conv1.kernel"], p["u1.conv1.bias"]))))
    sc, sh, _ = IR.folded_formula(bn_of(p, "u1.norm1"))
    (got,) = IR._conv2d_up2(dict(x=low, w=p["u1.conv1.kernel"], bias=p["u1.conv1.bias"], act1=RELU, scale=sc, shift=sh, act2=RELU, proj=None))
    close(got, up, "up block")
    # the skip layer: the second source scaled (0.25 here: exact in fp32, the oracle applies its own 1 / 255 in float64)
    sk = rng.normal(size=up.shape)
    close(IR._conv2d(conv_operands(x=up, x2=sk, x2_scale=0.25, w=p["s1.conv1.kernel"], bias=p["s1.conv1.bias"]))[0],
          ops.conv2d(np.concatenate([up, 0.25 * sk], axis=-1), p["s1.conv1.kernel"], p["s1.conv1.bias"]), "skip layer")


def test_composed_and_projected_tail_equals_the_oracles_three_layers(hal_small):
    """relu(BN(conv2(s1(concat[u1, d1 / 255])))) of the oracle equals (a) ONE 1x1 launch with the composed filter, `cout_valid` 3 and the
    folded norm2, and (b) the two projections out of the producing launches meeting in affine_act -- with the float64 formulas of
    inference_replay as the derived operands"""
    p = hal_small
    rng = np.random.default_rng(3)
    model = types.SimpleNamespace(s1=types.SimpleNamespace(conv1=types.SimpleNamespace(kernel=torch.from_numpy(p["s1.conv1.kernel"]),
                                                                                         bias=torch.from_numpy(p["s1.conv1.bias"]))),
                                  conv2=types.SimpleNamespace(kernel=torch.from_numpy(p["conv2.kernel"]), bias=torch.from_numpy(p["conv2.bias"])))
    wc, _, bc, _ = IR.tail_formula(model)
    sc, sh, _ = IR.folded_formula(bn_of(p, "norm2"))
    low, f = rng.normal(size=(1, 4, 6, 128)), rng.normal(size=(1, 8, 12, 64)) * 50.0
    u1 = ops.relu(ops.batch_norm_infer(ops.relu(ops.conv2d(ops.resize_bilinear_2x(low), p["u1.conv1.kernel"], p["u1.conv1.bias"])),
                                       *(p["u1.norm1" + s] for s in (".gamma", ".beta", ".moving_mean", ".moving_variance"))))
    d1 = ops.relu(ops.conv2d(f, p["d1.conv2.kernel"], p["d1.conv2.bias"]))
    s1 = ops.conv2d(np.concatenate([u1, d1 * (1.0 / 255)], axis=-1), p["s1.conv1.kernel"], p["s1.conv1.bias"])
    want = ops.relu(ops.batch_norm_infer(ops.conv2d(s1, p["conv2.kernel"], p["conv2.bias"]),
                                         *(p["norm2" + s] for s in (".gamma", ".beta", ".moving_mean", ".moving_variance"))))
    w16 = np.zeros((1, 1, 128, 16))
    w16[0, 0, :, :3] = wc
    close(IR._conv2d(conv_operands(x=u1, x2=d1, w=w16, bias=bc, cout_valid=3, scale=pad(sc, 0, 16), shift=pad(sh, 0, 16), act2=RELU))[0], want, "composed tail")
    m = (wc * sc).T
    su, sh1 = IR.folded_formula(bn_of(p, "u1.norm1"))[:2]
    (pu,) = IR._conv2d_up2(dict(x=low, w=p["u1.conv1.kernel"], bias=p["u1.conv1.bias"], act1=RELU, scale=su, shift=sh1, act2=RELU, proj=m[:, :64]))
    pd, pooled = IR._conv2d_maxpool2(dict(x=f, w=p["d1.conv2.kernel"], bias=p["d1.conv2.bias"], act1=RELU, keep_y=True, proj=m[:, 64:]))
    close(pooled, ops.max_pool(d1, 2, 2), "pooled beside the projection")
    close(IR.OPS["affine_act"].ref(dict(x=pu, scale=None, shift=sc * bc + sh, residual=pd, act=RELU))[0], want, "projected tail")


def test_elementwise_references_equal_the_oracle():
    rng = np.random.default_rng(4)
    x = rng.random((2, 6, 8, 3))
    x[0, :2] = 1.0
    hal = rng.random((2, 6, 8, 3))
    A, alpha = IR.OPS["alpha_blend"].ref(dict(b_pred=x, hal_bgr=hal, thr=0.125, return_alpha=True))     # (a threshold fp32 holds exactly)
    close(A, ops.alpha_blend(x, hal, 0.125), "alpha_blend")
    assert alpha.shape == (2, 6, 8, 1) and alpha.max() == 1.0
    close(IR.OPS["pack3"].ref(dict(srcs=[x, hal], out_channels=8, dtype=None))[0], pad(np.concatenate([x, hal], -1), 3, 8), "pack3")
    close(IR.OPS["vgg_preprocess"].ref(dict(x=x, out_channels=4, dtype=None))[0], pad(ops.vgg_preprocess(x), 3, 4), "vgg_preprocess")
    close(IR.OPS["lin_frontend"].ref(dict(img=x, channels=96, dtype=None))[0], pad(ops.lin_frontend(x), 3, 96), "lin_frontend")
    close(IR.OPS["clip"].ref(dict(x=x * 2 - 0.5, lo=0.0, hi=1.0))[0], np.clip(x * 2 - 0.5, 0, 1), "clip")
    rf = np.cumsum(rng.random((2, 1024)), axis=1)
    rf = (rf - rf[:, :1]) / (rf[:, -1:] - rf[:, :1])
    xs = np.round(x * 255) / 255 * 0.999
    close(IR.OPS["apply_rf"].ref(dict(x=xs, rf=rf))[0], ops.apply_rf(xs, rf), "apply_rf")
    close(IR.OPS["increase"].ref(dict(rf=rf - 0.3 * rng.random(rf.shape)))[0].shape, (2, 1024))
    assert IR.OPS["fork"].ref(dict(x=x, n=3))[2] is x and IR.OPS["mark"].ref(dict(x=x, callback=None))[0] is x


def test_every_entry_point_the_issue_names_has_a_reference_and_the_bars_are_the_projects():
    named = ("conv2d conv2d_up2 conv2d_maxpool2 conv2d_avgpool2 affine_act add clip vgg_preprocess pack3 alpha_blend apply_rf lin_frontend "
             "soft_hist invcrf_decode increase maxpool3s2 global_avg_pool avgpool2 resize2x reverse3 fork mark").split()
    assert set(named) <= set(IR.OPS)
    K = importlib.import_module("singlehdr-tf2_amd._ops")
    assert all(callable(getattr(K, n)) for n in IR.OPS)
    f16, f32 = torch.float16, torch.float32
    plain = dict(cout_valid=None, w=torch.zeros(1, 1, 128, 16), x2=None, shift=None, act2=0)
    L = lambda op, dt, **a: types.SimpleNamespace(op=op, dtype=dt, a=dict(plain, **a))      # noqa: E731
    O = lambda dt: types.SimpleNamespace(dtype=dt)                 # noqa: E731
    assert IR.bar_of(L("conv2d", f32), O(f32), "out[0]")[0] == 1e-5 == IR.bar_of(L("conv2d_maxpool2", f32), O(f32), "pooled")[0]
    assert IR.bar_of(L("conv2d_up2", f32), O(f32), "proj")[0] == IR.UF.TOL
    assert IR.bar_of(L("conv2d", f16), O(f16), "out[0]") == TP.bar_of("Conv2dHFn", "conv", True, f16) == IR.bar_of(L("conv2d", f16), O(f32), "out[0]")
    assert IR.bar_of(L("affine_act", f32), O(f32), "out[0]")[0] == 1e-5 and IR.bar_of(L("increase", f32), O(f32), "out[0]")[0] == 2e-4
    assert IR.bar_of(L("avgpool2", f16), O(f16), "out[0]")[0] == 2.0 ** -10
    # the one measured bar: the composed Hallucination tail in native fp16, and nothing else
    tail = dict(cout_valid=3, x2=torch.zeros(1), shift=torch.zeros(16), act2=RELU)
    assert IR.bar_of(L("conv2d", f16, **tail), O(f32), "out[0]")[0] == IR.FP16_TAIL_BAR == 2.0 ** -5 > 2 * 9.272e-3 > 2.0 ** -6
    assert IR.bar_of(L("conv2d", f32, **tail), O(f32), "out[0]")[0] == 1e-5
    assert IR.bar_of(L("conv2d", f16, **dict(tail, x2=None)), O(f32), "out[0]")[0] == 2e-3 == IR.bar_of(L("conv2d", f16, **dict(tail, act2=0)), O(f32), "out[0]")[0]


# ---- 2. the derived operands on CPU models -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_models():
    cpu = torch.device("cpu")
    shdr = importlib.import_module("singlehdr-tf2_amd")
    hal = shdr.hallucination_net.model(device=cpu).load_numpy(nets.init_params(nets.hal_spec(), 31))
    lin = shdr.linearization_net.model(device=cpu).load_numpy(nets.init_params(nets.lin_spec(), 32))
    return shdr, {"hal": hal, "lin": lin}


def build_derived(models):
    hal, lin = models["hal"], models["lin"]
    for m in models.values():
        m._drop_derived()
        for _, layer in IR._walk(m):
            if hasattr(layer, "_folded"):
                layer._folded = None
                layer.folded()
    hal.d1.conv1.kernel_padded(cin_pad=4)
    lin.crf_feature_net.conv1.kernel_padded(cin_pad=96)
    hal._tail_filter(64)
    assert hal._tail_projection() is not None
    return IR.derived_catalog(models)


def test_derived_operands_meet_their_counted_bars_on_cpu_models(cpu_models):
    _, models = cpu_models
    cat = build_derived(models)
    entries = [d.compare() for d in cat.values()]
    names = {e.name for e in entries}
    print("\n".join(e.line() for e in entries if "res" not in e.name))
    assert len([n for n in names if n.endswith(".folded.scale")]) == 7 + 1 + 4 + 3 + 3 + 4 + 3 == len([n for n in names if n.endswith(".folded.shift")])
    assert {"hal.d1.conv1.kernel_padded", "lin.crf_feature_net.conv1.kernel_padded", "hal._tail_filter.wc", "hal._tail_filter.bc",
            "hal._tail_projection.up_map", "hal._tail_projection.skip_map", "hal._tail_projection.const", "hal._tail_projection.up_filter"} <= names
    assert all(e.ok for e in entries), "\n".join(e.line() for e in entries if not e.ok)
    # the bars are tight enough to mean something: a relative error of 2^-17 in any of them is outside
    for d in cat.values():
        if d.name.endswith(("scale", "up_map", "const", ".bc")):
            assert not d.compare(d.tensor * (1.0 + 2.0 ** -17)).ok, d.name


def test_planted_fold_error_is_caught_at_the_shifts_and_what_is_built_from_them(cpu_models, monkeypatch):
    shdr, models = cpu_models
    BN = shdr._layers.BatchNormalization

    def wrong(self):
        with torch.no_grad():
            scale = self.gamma.detach() * torch.rsqrt(self.moving_variance + shdr._layers.BN_EPS)
            self._folded = (None, scale.contiguous(), (self.beta.detach() + self.moving_mean * scale).contiguous())
        return self._folded[1], self._folded[2]
    monkeypatch.setattr(BN, "folded", wrong)
    try:
        cat = build_derived(models)
        bad = {e.name for e in (d.compare() for d in cat.values()) if not e.ok}
        assert bad == {d.name for d in cat.values() if d.name.endswith(".folded.shift")} | {"hal._tail_projection.const"}, sorted(bad)
    finally:
        for m in models.values():
            m._drop_derived()
            for _, layer in IR._walk(m):
                if hasattr(layer, "_folded"):
                    layer._folded = None


# ---- 3. the recorder on a stub module ------------------------------------------------------------------------------------------------------
def make_stub(wrong_add=False):
    """a torch-CPU module with the call surface of `_ops` that the recorder touches: entry points that look each other up on the module at
    call time, `_lib.check`, PRECISION, and the range record"""
    S = types.ModuleType("stub_ops")
    S.PRECISION = "fp32"
    S.RANGE_MISSES = __import__("collections").Counter()
    S._lib = types.SimpleNamespace(check=lambda rc, name: None)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))      # noqa: E731

    def _record(t):
        return getattr(t, "_r", (None, None))

    def _set_range(t, slot, bound=None):
        t._r = (slot, bound)
        return t

    def _range_of(t):
        slot, b = S._record(t)
        return slot if slot is not None or b is None else torch.full((1,), b)

    def resize2x(x):
        S._lib.check(0, "stub_resize2x")
        return S._set_range(t32(IR.H.resize2x(TP.widen(x))), *S._record(x))      # convex: bounded by the input's bound

    def conv2d(x, w, bias=None, stride=1, x2=None, x2_scale=1.0, act1=0, scale=None, shift=None, residual=None, act2=0, algo=0, out=None,
               cout_valid=None, pad=None, out_hw=None, w_batch_stride=0):
        S._range_of(x)
        S._lib.check(0, "stub_conv2d")
        wd = lambda v: None if v is None else TP.widen(v)      # noqa: E731
        y = t32(IR.conv_chain(wd(x), wd(w), wd(bias), stride, wd(x2), x2_scale, act1, wd(scale), wd(shift), wd(residual), act2, cout_valid))
        return S._set_range(y, y.abs().max().reshape(1))

    def conv2d_up2(x, w, bias=None, act1=0, scale=None, shift=None, act2=0, proj=None, lowres=False, one_launch=False):
        if proj is not None:
            return None
        return S.conv2d(S.resize2x(x), w, bias, act1=act1, scale=scale, shift=shift, act2=act2)

    def conv2d_maxpool2(x, w, bias=None, act1=0, keep_y=True, proj=None):
        y = S.conv2d(x, w, bias, act1=act1)
        S._lib.check(0, "stub_maxpool2")
        return y, S._set_range(t32(IR.H.maxpool2(TP.widen(y))), *S._record(y))

    def clip(x, lo, hi):
        S._lib.check(0, "stub_clip")
        y = torch.clamp(x, lo, hi)
        y._r = (None, max(abs(lo), abs(hi)))
        return y

    def add(a, b, relu=False):
        S._lib.check(0, "stub_add")
        return a + b * (1.001 if wrong_add else 1.0)

    def fork(x, n=2):
        return (x,) * n
    for f in (_record, _set_range, _range_of, resize2x, conv2d, conv2d_up2, conv2d_maxpool2, clip, add, fork):
        setattr(S, f.__name__, f)
    return S, t32


def stub_pass(S, t32, gap=False):
    rng = np.random.default_rng(9)
    x = t32(rng.normal(size=(1, 4, 6, 8)))
    w = t32(rng.normal(size=(3, 3, 8, 16)) / 8.0)
    with IR.record(S, audit=True) as rec:
        a, b = S.fork(S.clip(x, -1.0, 1.0))
        assert S.conv2d_up2(a, w, proj=t32(np.ones((3, 16)))) is None
        u = S.conv2d_up2(a, w, act1=RELU)
        y, yp = S.conv2d_maxpool2(b, w, act1=LRELU)
        if gap:
            yp = yp * 2.0                                            # an op between two recorded ops
        S._lib.check(0, "stub_outside")
        w1 = t32(rng.normal(size=(1, 1, 16, 16)) / 4.0)
        out = S.add(S.conv2d(yp, w1), yp)
        S.conv2d(u, w1)
    return rec, x, u, out


def test_recorder_nesting_snapshots_returns_and_the_closed_chain():
    S, t32 = make_stub()
    orig = {n: getattr(S, n) for n in ("conv2d", "add", "_range_of", "_set_range")}
    rec, x, u, out = stub_pass(S, t32)
    assert all(getattr(S, n) is f for n, f in orig.items()) and S._lib.check(0, "x") is None                 # restored
    assert [l.op for l in rec.launches] == ["clip", "fork", "conv2d_up2", "conv2d_up2", "conv2d_maxpool2", "conv2d", "add", "conv2d"]
    none, up, pool = rec.launches[2], rec.launches[3], rec.launches[4]
    assert none.form == "none" and none.outs == () and none.children == []
    assert [c.op for c in up.children] == ["resize2x", "conv2d"] and up.form == "single" and up.outs[0] is u
    assert [c.op for c in pool.children] == ["conv2d"] and pool.form == "tuple" and len(pool.outs) == 2
    assert rec.launches[1].form == "tuple" and rec.launches[1].outs[0] is rec.launches[1].outs[1]
    assert [l.idx for l in rec.all()] == sorted(l.idx for l in rec.all()) and len(list(rec.all())) == 11
    # C ABI names: inside a launch they belong to it and to the launch around it, outside they are listed
    assert up.abi == ["stub_resize2x", "stub_conv2d"] and up.children[0].abi == ["stub_resize2x"] and rec.outside == ["stub_outside"]
    assert rec.abi_names() == {"stub_clip", "stub_resize2x", "stub_conv2d", "stub_maxpool2", "stub_add"}
    # snapshots: an input buffer rewritten after the pass changes nothing that is replayed
    clip = rec.launches[0]
    assert clip.live["x"] is x and clip.a["x"] is not x
    x.mul_(3.0)
    assert not torch.equal(clip.a["x"], x)
    rep = IR.replay(rec)
    rep.assert_ok()
    assert len(rep.entries) == 1 + 2 + 1 + 2 + 1 + 1 + 1 and {e.item for e in rep.entries} == {"out[0]", "out[1]", "y", "pooled"}
    assert IR.open_inputs(rec, [clip.a["x"]]) == []
    assert [(l.op, n) for l, n in IR.open_inputs(rec, [])] == [("clip", "x")]


def test_planted_gap_and_planted_wrong_launch_are_reported_exactly():
    S, t32 = make_stub()
    rec, _, _, _ = stub_pass(S, t32, gap=True)
    IR.replay(rec).assert_ok()
    assert [(l.op, n) for l, n in IR.open_inputs(rec, [rec.launches[0].a["x"]])] == [("conv2d", "x"), ("add", "b")]
    S, t32 = make_stub(wrong_add=True)
    rec, _, _, _ = stub_pass(S, t32)
    rep = IR.replay(rec)
    assert rep.failed() == {(rec.of("add")[0].idx, "out[0]")}
    with pytest.raises(AssertionError, match="1 of 9 comparisons"):
        rep.assert_ok()


def test_range_audit_on_the_stub():
    """kernel-written slots must equal the maximum of the tensor they were written for, host bounds must bound it; a halved host bound is
    reported at exactly its consumer"""
    S, t32 = make_stub()
    rec, _, _, _ = stub_pass(S, t32)
    aud = rec.audit.finish()
    kinds = [(c.who, c.kind, c.exact) for c in aud.items]
    # (the pooled tensor carries the slot written for y: sound, not exact; u is consumed with the slot written for it)
    assert kinds == [("conv2d", "host", False)] * 2 + [("conv2d", "slot", False), ("conv2d", "slot", True)], kinds
    aud.assert_sound()
    assert aud.misses() == {} and "conv2d" in aud.summary()
    S.clip = lambda x, lo, hi: S._set_range(torch.clamp(x, lo, hi), None, 0.25)
    rec, _, _, _ = stub_pass(S, t32)
    bad = rec.audit.finish().failures()
    assert [(c.who, c.kind) for c in bad] == [("conv2d", "host")] * 2 and all(c.consumed == 0.25 < c.actual for c in bad)
    with pytest.raises(AssertionError, match="2 of 4 consumptions"):
        rec.audit.assert_sound()
