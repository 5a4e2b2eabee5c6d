"""Replay of a recorded autograd tape, node by node, against float64 local references -- test infrastructure.

A whole-net gradient bar has to be wide: the fp32 forward differs from a float64 reference by ~1e-6, a few relu / max-pool / `_increase`
masks flip, and the gradient moves at the percent level (tests/test_gpu_grad.py::test_training_gradients_are_mask_flip_sensitive).  A
mask flip is a property of the INPUT of a node, not of the node.  So this module records every `torch.autograd.Function` call of
`_autograd.py` during one forward and backward pass -- the device's own inputs, outputs, upstream gradient and returned gradients of
every node -- and compares each node with a float64 statement of that node alone, fed the device's operands.  The op-level bars of
the project (1e-5 / 1e-4 fp32, 2e-3 / 3e-3 fp16) then hold for every node of the real nets, and a failure names the node.

  record(A)                 context manager: wraps `.apply` of every Function subclass found in module A (by introspection) and, through
                            `grad_fn.register_hook`, captures each node's grad_outputs / grad_inputs during backward
  REFS                      class name -> Ref(forward, vjp, kind): float64, NumPy / torch-CPU, nothing of the package under test
  replay(rec, variables)    the comparison: per node forward and every non-None grad_input; per variable `p.grad` against the SUM of the
                            float64 local parameter gradients over all nodes that consume it (covers the `_acc` fast path, which returns
                            None and adds into the flat buffer)
  cut_edges / foreign_nodes / unforked_fanouts      structure checks on the same recording

Decisions (activation masks, max-pool routing, clip, `_increase`, soft bins, alpha live-ness, the CRF table knot) are taken from the
recorded operands exactly as the kernels take them; no element is excluded from any comparison.  Importing this module needs no GPU.
"""
import contextlib

import numpy as np
import torch

import fp16_ref as H
import tape_ref as TR
import torch_ref as R

ACT_RELU = 1
ULP16 = 2.0 ** -10        # one fp16 ulp relative to the binade's lower end: the bar of an fp16 elementwise twin, tensor-relative

# ---- bars: the project's existing op-level bars (tests/test_gpu_grad.py, tests/test_gpu_fp16_oracle.py) ------------
FWD32 = {"conv": 1e-5, "bn": 1e-5, "glue": 1e-5, "crf": 2e-4}
GRAD32 = {"conv": 1e-4, "bn": 1e-4, "glue": 1e-5, "crf": 2e-4}
CONV16_FWD, CONV16_GRAD = 2e-3, 3e-3
MODEL_SCALE = 1e-3        # a parameter gradient that vanishes identically is measured against 1e-3 of the model-wide maximum (_grad_check)


def f32c(v):
    """a host constant as the kernels receive it: rounded to fp32"""
    return float(np.float32(v))


def widen(t):
    """device (or host) tensor -> float64 ndarray, exactly"""
    return t.detach().to("cpu", torch.float64).numpy()


# ---- the recorder ------------------------------------------------------------------------------------------------------------------
class Node:
    """one `.apply` call: cls, args (tensors by reference, the rest by value), outs (tuple), prec (K.PRECISION at call time),
    arg_requires_grad (as the arguments arrived), grad_outputs / grad_inputs (filled by the node hook during backward)"""

    def __init__(self, idx, cls, args, outs, single, prec):
        self.idx, self.cls, self.args, self.outs, self.single, self.prec = idx, cls, list(args), outs, single, prec
        self.arg_requires_grad = [isinstance(a, torch.Tensor) and a.requires_grad for a in args]
        self.grad_outputs = self.grad_inputs = None
        self.grad_fn = next((o.grad_fn for o in outs if isinstance(o, torch.Tensor) and o.grad_fn is not None), None)
        self.hook_calls = 0

    @property
    def name(self):
        return self.cls.__name__

    def aligned_grad_inputs(self):
        """grad_inputs aligned with args: the hook of a node sees one entry per TENSOR argument (the edges of the node), in order"""
        pos = [j for j, a in enumerate(self.args) if isinstance(a, torch.Tensor)]
        assert len(self.grad_inputs) == len(pos), (self.name, len(self.grad_inputs), len(pos))
        out = [None] * len(self.args)
        for j, g in zip(pos, self.grad_inputs):
            out[j] = g
        return out

    def shapes(self):
        return [tuple(a.shape) for a in self.args if isinstance(a, torch.Tensor)]


def function_classes(module):
    """every torch.autograd.Function subclass that lives in `module`, found by introspection"""
    return [v for v in vars(module).values()
            if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v is not torch.autograd.Function]


class Recording:
    def __init__(self, module):
        self.module = module
        self.nodes = []
        self.roots = []           # tensors `.backward()` was called on while recording

    def of(self, name):
        return [n for n in self.nodes if n.name == name]


@contextlib.contextmanager
def record(module, precision_of=None):
    """with record(A) as rec: <forward and backward>.  precision_of: callable returning the precision to store per node (default:
    module.K.PRECISION).  The product code is untouched: `.apply` is shadowed on each subclass and restored on exit."""
    rec = Recording(module)
    classes = function_classes(module)
    if precision_of is None:
        precision_of = lambda: getattr(getattr(module, "K", None), "PRECISION", None)    # noqa: E731

    def wrap(cls):
        inherited = cls.apply                                   # bound classmethod of torch.autograd.Function

        def apply(*args):
            out = inherited(*args)
            single = not isinstance(out, tuple)
            node = Node(len(rec.nodes), cls, args, (out,) if single else tuple(out), single, precision_of())
            rec.nodes.append(node)
            if node.grad_fn is not None:
                def hook(grad_inputs, grad_outputs, node=node):
                    node.hook_calls += 1
                    node.grad_inputs, node.grad_outputs = tuple(grad_inputs), tuple(grad_outputs)
                node.grad_fn.register_hook(hook)
            return out
        return staticmethod(apply)

    shadowed = []
    tensor_backward = torch.Tensor.backward

    def backward(self, *a, **kw):
        rec.roots.append(self)
        return tensor_backward(self, *a, **kw)
    try:
        for cls in classes:
            assert "apply" not in vars(cls), "%s defines its own apply" % cls.__name__
            cls.apply = wrap(cls)
            shadowed.append(cls)
        torch.Tensor.backward = backward
        yield rec
    finally:
        torch.Tensor.backward = tensor_backward
        for cls in shadowed:
            del cls.apply


# ---- float64 local references ------------------------------------------------------------------------------------------------------
def act(v, a):
    return TR.act(v, a)


def conv_linear(xin, w, stride):
    """SAME-padded convolution without bias, float64 (engine: torch-CPU conv2d, pinned to the oracle through torch_ref.conv2d)"""
    with torch.no_grad():
        return R.conv2d(R.T(xin), R.T(w), None, stride).numpy()


def conv_linear_vjp(xin, w, stride, dz):
    """(d xin, d w) of sum(conv_linear(xin, w) * dz): the transpose of a LINEAR map, taken by the same engine"""
    tx, tw = R.T(xin, True), R.T(w, True)
    gx, gw = torch.autograd.grad(R.conv2d(tx, tw, None, stride), [tx, tw], R.T(dz))
    return gx.numpy(), gw.numpy()


def _conv_operands(x, x2, w, bias, x2_scale, cout_valid):
    s = f32c(x2_scale)
    cv = cout_valid or w.shape[3]
    xin = x if x2 is None else np.concatenate([x, s * x2], axis=-1)
    b = None if bias is None else bias[:cv]
    return xin, w[..., :cv], b, s, cv


def conv_fwd(x, x2, w, bias, stride, x2_scale, act1, cout_valid, *_):
    """y = act1(conv(concat[x, x2_scale x2], w[..., :cout_valid]) + bias)"""
    xin, wv, b, _, _ = _conv_operands(x, x2, w, bias, x2_scale, cout_valid)
    z = conv_linear(xin, wv, stride)
    return (act(z if b is None else z + b, act1),)


def conv_vjp(args, y, g):
    """(dx, dx2, dw, db): the activation mask from the device's y; dw zero in the padded columns; dx2 carries x2_scale"""
    x, x2, w, bias, stride, x2_scale, act1, cout_valid = args[:8]
    xin, wv, _, s, cv = _conv_operands(x, x2, w, bias, x2_scale, cout_valid)
    dz = H.act_grad(g[0], y[0], act1)
    dxin, dwv = conv_linear_vjp(xin, wv, stride, dz)
    c1 = x.shape[3]
    dw = np.zeros(w.shape)
    dw[..., :cv] = dwv
    db = None
    if bias is not None:
        db = np.zeros(bias.shape)
        db[:cv] = dz.reshape(-1, cv).sum(axis=0)
    dx2 = None if x2 is None else s * dxin[..., c1:]
    return (dxin[..., :c1], dx2, dw, db) + (None,) * (len(args) - 4)


def bn_train_fwd(x, gamma, beta, mm, mv, eps, momentum, relu):
    mean, var = H.bn_stats(x)
    return (H.bn_apply(x, mean, var, gamma, beta, f32c(eps), relu),)


def bn_train_vjp(args, y, g):
    x, gamma, beta, _, _, eps, _, relu = args
    mean, var = H.bn_stats(x)
    dx, dgamma, dbeta = H.bn_bwd(g[0], x, y[0] if relu else None, mean, var, gamma, f32c(eps))
    return (dx, dgamma, dbeta, None, None, None, None, None)


def bn_frozen_fwd(x, gamma, beta, mean, var, eps, residual, a):
    v = (x - mean) / np.sqrt(var + f32c(eps)) * gamma + beta
    return (act(v if residual is None else v + residual, a),)


def bn_frozen_vjp(args, y, g):
    """the moving statistics are constants: dx = d gamma rstd, dgamma = sum d (x - mean) rstd, dbeta = sum d, dresidual = d"""
    x, gamma, beta, mean, var, eps, residual, a = args
    d = H.act_grad(g[0], y[0], a)
    rstd = 1.0 / np.sqrt(var + f32c(eps))
    c = x.shape[-1]
    return (d * gamma * rstd, (d * (x - mean) * rstd).reshape(-1, c).sum(axis=0), d.reshape(-1, c).sum(axis=0), None, None, None,
            None if residual is None else d, None)


def affine_act_vjp(args, y, g):
    x, scale, shift, residual, a = args
    d = H.act_grad(g[0], y[0], a)
    return (d if scale is None else d * scale, None, None, None if residual is None else d, None)


def maxpool2_bwd(x, dy):
    """first maximum of each complete window; the last row / column of an odd size belongs to no window"""
    n, h, w, c = x.shape
    dx = np.zeros(x.shape)
    dx[:, :h // 2 * 2, :w // 2 * 2] = H.maxpool2_bwd(x[:, :h // 2 * 2, :w // 2 * 2], dy)
    return dx


def increase_bwd(rf, dout):
    """tape_ref.increase_bwd with the two decisions -- is the smallest slope negative, and where is it -- taken on the fp32 differences
    the kernel forms (r[k + 1] - r[k] rounded to fp32); the values stay float64"""
    g32 = (rf[:, 1:].astype(np.float32) - rf[:, :-1].astype(np.float32)).astype(np.float64)
    g = rf[:, 1:] - rf[:, :-1]
    arg = g32.argmin(axis=1)
    rows = np.arange(rf.shape[0])
    mn = g[rows, arg]
    neg = g32[rows, arg] < 0.0
    ng = g + np.where(neg, -mn, 0.0)[:, None]
    S = ng.sum(axis=1, keepdims=True)
    dn = np.cumsum(dout[:, :0:-1], axis=1)[:, ::-1]
    d = dn / S - (dn * ng).sum(axis=1, keepdims=True) / (S * S)
    d[rows, arg] -= np.where(neg, d.sum(axis=1), 0.0)
    drf = np.zeros_like(rf)
    drf[:, 1:] += d
    drf[:, :-1] -= d
    return drf


def _rf_parts(x, K):
    """(yv, i0, i1, w0, w1): the knot floor(yv) from the fp32 product (K - 1) x as the kernels round it, the weights from the exact
    product -- the segment the device chose, extended linearly (the look-up is continuous at a knot)"""
    b = x.shape[0]
    xf = x.reshape(b, -1)
    y0 = np.floor((np.float32(K - 1) * xf.astype(np.float32)).astype(np.float64))
    yv = (K - 1.0) * xf
    i0 = np.clip(y0.astype(np.int64), 0, K - 1)
    i1 = np.clip(y0.astype(np.int64) + 1, 0, K - 1)
    return yv, i0, i1, (y0 + 1.0) - yv, yv - y0


def apply_rf_fwd(x, rf):
    _, i0, i1, w0, w1 = _rf_parts(x, rf.shape[1])
    return ((w0 * np.take_along_axis(rf, i0, 1) + w1 * np.take_along_axis(rf, i1, 1)).reshape(x.shape),)


def apply_rf_vjp(args, y, g):
    x, rf = args
    b, K = rf.shape
    _, i0, i1, w0, w1 = _rf_parts(x, K)
    gg = g[0].reshape(b, -1)
    drf = np.zeros_like(rf)
    rows = np.broadcast_to(np.arange(b)[:, None], i0.shape)
    np.add.at(drf, (rows, i0), gg * w0)
    np.add.at(drf, (rows, i1), gg * w1)
    dx = gg * (K - 1.0) * (np.take_along_axis(rf, i1, 1) - np.take_along_axis(rf, i0, 1))
    return (dx.reshape(x.shape), drf)


def fork_vjp(args, y, g):
    live = [t for t in g if t is not None]
    return (sum(live[1:], live[0]) if live else None, None)


def unpack3_vjp(args, y, g):
    yin, nout = args
    zero = np.zeros(yin.shape[:-1] + (3,))
    return (H.pack3([zero if t is None else t for t in g], yin.shape[-1]), None)


def mean_norm_fwd(r, eps, target):
    return (TR.mean_norm_fwd(r, TR.sample_dot(r), f32c(eps), f32c(target)),)


def mean_norm_vjp(args, y, g):
    r, eps, target = args
    return (TR.mean_norm_bwd(g[0], TR.sample_dot(r), TR.sample_dot(g[0], r), f32c(eps), f32c(target)), None, None)


class Ref:
    """fwd(*args) -> tuple of float64 outputs; vjp(args, y, g) -> tuple aligned with args (None: no gradient); args / y / g are the
    recorded operands widened to float64 (non-tensors as they were), y the DEVICE's outputs"""

    def __init__(self, kind, fwd, vjp):
        self.kind, self.fwd, self.vjp = kind, fwd, vjp


def _g1(fn):
    """vjp of a one-input op from bwd(args, y, dy) -> dx; the other arguments get None"""
    return lambda args, y, g: (fn(args, y, g[0]),) + (None,) * (len(args) - 1)


REFS = {
    "Conv2dFn": Ref("conv", conv_fwd, conv_vjp),
    "Conv2dHFn": Ref("conv", conv_fwd, conv_vjp),
    "BatchNormTrainFn": Ref("bn", bn_train_fwd, bn_train_vjp),
    "BatchNormFrozenFn": Ref("bn", bn_frozen_fwd, bn_frozen_vjp),
    "AffineActFn": Ref("bn", lambda x, sc, sh, res, a: (TR.affine_act(x, sc, sh, res, a),), affine_act_vjp),
    "AvgPool2Fn": Ref("glue", lambda x: (H.avgpool2(x),), _g1(lambda a, y, dy: H.avgpool2_bwd(dy, a[0].shape))),
    "MaxPool2Fn": Ref("glue", lambda x: (H.maxpool2(x),), _g1(lambda a, y, dy: maxpool2_bwd(a[0], dy))),
    "MaxPool3s2Fn": Ref("glue", lambda x: (H.maxpool3s2(x),), _g1(lambda a, y, dy: H.maxpool3s2_bwd(a[0], dy))),
    "Resize2xFn": Ref("glue", lambda x: (H.resize2x(x),), _g1(lambda a, y, dy: H.resize2x_bwd(dy, a[0].shape))),
    "GapFn": Ref("glue", lambda x: (H.gap(x),), _g1(lambda a, y, dy: H.gap_bwd(dy, a[0].shape))),
    "ClipFn": Ref("glue", lambda x, lo, hi: (TR.clip(x, f32c(lo), f32c(hi)),),
                  _g1(lambda a, y, dy: TR.clip_bwd(dy, a[0], f32c(a[1]), f32c(a[2])))),
    "LogcFn": Ref("glue", lambda x: (TR.logc(x),), _g1(lambda a, y, dy: TR.logc_bwd(dy, a[0]))),
    "Reverse3Fn": Ref("glue", lambda x: (TR.reverse3(x),), _g1(lambda a, y, dy: TR.reverse3(dy))),
    "VggPreFn": Ref("glue", lambda x, oc, dt: (TR.vgg_preprocess(x, oc),), _g1(lambda a, y, dy: TR.vgg_preprocess_bwd(dy))),
    "IncreaseFn": Ref("crf", lambda rf: (TR.increase(rf),), _g1(lambda a, y, dy: increase_bwd(a[0], dy))),
    "AddFn": Ref("glue", lambda a, b: (a + b,), lambda args, y, g: (g[0], g[0])),
    "AddReluFn": Ref("glue", lambda a, b: (np.maximum(a + b, 0.0),),
                     lambda args, y, g: (H.act_grad(g[0], y[0], ACT_RELU),) * 2),
    "ForkFn": Ref("glue", lambda x, n: (x,) * n, fork_vjp),
    "MarkFn": Ref("glue", lambda x, cb: (x,), lambda args, y, g: (g[0], None)),
    "InvcrfDecodeFn": Ref("crf", lambda feat, wfc, bfc, table: (TR.invcrf_decode(feat, wfc, bfc, table),),
                          lambda args, y, g: TR.invcrf_decode_bwd(g[0], args[0], args[1], args[3]) + (None,)),
    "ApplyRfFn": Ref("crf", apply_rf_fwd, apply_rf_vjp),
    "DiffLossFn": Ref("glue", lambda a, b, mode: (TR.diff_loss(a, b, mode),),
                      lambda args, y, g: (TR.diff_loss_bwd(args[0], args[1], g[0], args[2]),
                                          TR.diff_loss_bwd(args[1], args[0], g[0], args[2]), None)),
    "TvLossFn": Ref("glue", lambda y: (np.array([TR.tv_loss(y)]),), _g1(lambda a, y, dy: TR.tv_loss_bwd(a[0], dy))),
    "BlendConstFn": Ref("glue", lambda base, alpha, hal, thr: (TR.alpha_blend(base, hal, f32c(thr))[0],),
                        lambda args, y, g: (None, None, TR.alpha_blend_bwd(g[0], args[1]), None)),
    "LinFrontendFn": Ref("glue", lambda img, ch, dt: (H.lin_frontend(img, ch),), _g1(lambda a, y, dy: H.lin_frontend_bwd(a[0], dy))),
    "AlphaBlendFn": Ref("glue", lambda b, hal, thr: (TR.alpha_blend(b, hal, f32c(thr))[0],),
                        lambda args, y, g: TR.alpha_blend_full_bwd(args[0], args[1], g[0], f32c(args[2])) + (None,)),
    "Pack3Fn": Ref("glue", lambda oc, dt, *srcs: (H.pack3(srcs, oc),),
                   lambda args, y, g: (None, None) + tuple(H.unpack3(g[0], len(args) - 2))),
    "Unpack3Fn": Ref("glue", lambda y, nout: tuple(H.unpack3(y, nout)), unpack3_vjp),
    "MeanNormFn": Ref("glue", mean_norm_fwd, mean_norm_vjp),
}


# ---- bars per compared tensor -------------------------------------------------------------------------------------------------------
def bar_of(name, kind, is_forward, got_dtype):
    """(bar, label).  Conv2dHFn: the fp16 conv bars for every item (its fp32 parameter gradients come from fp16 operands); any other
    fp16 result: one fp16 ulp (the rounding of the stored value); an fp32 result: the fp32 bar of the node's kind"""
    if name == "Conv2dHFn":
        return (CONV16_FWD, "fp16 conv forward") if is_forward else (CONV16_GRAD, "fp16 dgrad / wgrad")
    if got_dtype == torch.float16:
        return ULP16, "fp16 elementwise twin"
    return ((FWD32 if is_forward else GRAD32)[kind], "fp32 %s %s" % (kind, "forward" if is_forward else "gradient"))


# ---- the replay ------------------------------------------------------------------------------------------------------------------------
class Entry:
    """one compared tensor: node index (or None for a variable), class name, item, shapes, plan / precision, abs error, reference
    maximum, bar, worst element"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.floor = 0.0

    @property
    def rel(self):
        return self.err / max(self.ref_max, self.floor, 1e-30)

    @property
    def ok(self):
        return self.rel <= self.bar

    def line(self):
        return "%s #%s %-17s %-9s %-26s %s  rel %.3e (bar %.0e, %s)  worst %s got %.9g want %.9g  ref max %.3e%s" % (
            "ok  " if self.ok else "FAIL", self.idx, self.name, self.item, self.plan, self.shapes, self.rel, self.bar, self.label, self.where,
            self.got, self.want, self.ref_max, "  floor %.3e" % self.floor if self.floor else "")


def _compare(got_t, want, **kw):
    got = widen(got_t)
    want = np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        if got.size != want.size:
            raise AssertionError("#%s %s %s: device shape %s, reference shape %s" % (kw["idx"], kw["name"], kw["item"], got.shape, want.shape))
        want = want.reshape(got.shape)
    d = np.abs(got - want)
    if not np.isfinite(d).all():
        d = np.where(np.isfinite(d), d, np.inf)
    k = int(np.argmax(d)) if d.size else 0
    where = tuple(int(i) for i in np.unravel_index(k, d.shape)) if d.size else ()
    return Entry(err=float(d.max()) if d.size else 0.0, ref_max=float(np.abs(want).max()) if d.size else 0.0, where=where,
                 got=float(got.reshape(-1)[k]) if d.size else 0.0, want=float(want.reshape(-1)[k]) if d.size else 0.0, **kw)


def variable_of(t):
    """the trainable leaf a tensor argument stands for: the leaf itself, or the leaf behind a zero-padding of it (Conv2D.call_padded
    pads a narrow filter on the tape); None for anything else"""
    if not isinstance(t, torch.Tensor) or not t.requires_grad:
        return None
    if t.is_leaf:
        return t
    fn = t.grad_fn
    if fn is not None and type(fn).__name__.startswith("ConstantPadNd"):
        nxt = fn.next_functions[0][0]
        if nxt is not None and type(nxt).__name__ == "AccumulateGrad":
            return nxt.variable
    return None


def _vkey(t):
    return (t.data_ptr(), tuple(t.shape))


def _crop(a, shape):
    return a[tuple(slice(0, s) for s in shape)]


class Report:
    def __init__(self):
        self.entries, self.var_entries, self.unconsumed, self.no_grad = [], [], [], []

    def failures(self):
        return [e for e in self.entries + self.var_entries if not e.ok]

    def failed_items(self):
        """{(node index, item)} of failing node entries, {variable name} of failing variables"""
        return ({(e.idx, e.item) for e in self.entries if not e.ok}, {e.item for e in self.var_entries if not e.ok})

    def worst_by_class(self):
        """{(class, label): (worst relative error, bar)}"""
        out = {}
        for e in self.entries + self.var_entries:
            k = (e.name, e.label + (" (on the model-wide scale)" if e.floor > e.ref_max else ""))
            if k not in out or e.rel > out[k][0]:
                out[k] = (e.rel, e.bar)
        return out

    def text(self, only_failures=False):
        rows = [e.line() for e in self.entries + self.var_entries if not (only_failures and e.ok)]
        rows += ["variable %s is consumed by no recorded node" % n for n in self.unconsumed]
        rows += ["variable %s ends without a gradient" % n for n in self.no_grad]
        return "\n".join(rows)

    def summary(self):
        return "\n".join("%-18s %-50s worst %.3e  bar %.0e" % (k[0], k[1], v[0], v[1]) for k, v in sorted(self.worst_by_class().items()))

    def closest(self, k=3):
        """the k comparisons that use the largest share of their bar"""
        rows = sorted(self.entries + self.var_entries, key=lambda e: -e.rel / e.bar)[:k]
        return "\n".join("  %4.2f of its bar: %s" % (e.rel / e.bar, e.line()) for e in rows)

    def assert_ok(self, leave=None):
        """leave(entry) -> True: a comparison that another test asserts at the same bar (it stays in the report)"""
        bad = [e for e in self.failures() if leave is None or not leave(e)]
        if bad or self.unconsumed or self.no_grad:
            raise AssertionError("tape replay: %d of %d comparisons outside their bar\n%s" % (
                len(bad), len(self.entries) + len(self.var_entries), self.text(only_failures=True)))


def replay(rec, variables=(), grad_scale=1.0, plan_of=None):
    """Compare every node of `rec` with its float64 local reference, and every variable's `.grad` with grad_scale times the sum of its
    float64 local gradients.  variables: [(name, tensor)] of the trainable variables (each must be consumed and end with a gradient).
    plan_of(node) -> str: the kernel plan of a convolution node, for the report.  A class without a reference raises KeyError."""
    rep = Report()
    expected, contributors = {}, {}
    var_names = {_vkey(t): n for n, t in variables}
    param_entries = []
    for node in rec.nodes:
        if node.name not in REFS:
            raise KeyError("no float64 reference registered for %s (node #%d): every Function class of the tape needs one" % (node.name, node.idx))
        ref = REFS[node.name]
        a64 = [widen(a) if isinstance(a, torch.Tensor) else a for a in node.args]
        plan = (plan_of(node) if plan_of is not None else None) or str(node.prec)
        common = dict(idx=node.idx, name=node.name, shapes=node.shapes(), plan=plan)
        want = ref.fwd(*a64)
        assert len(want) == len(node.outs), (node.name, len(want), len(node.outs))
        for j, (o, wv) in enumerate(zip(node.outs, want)):
            bar, label = bar_of(node.name, ref.kind, True, o.dtype)
            rep.entries.append(_compare(o, wv, item="fwd[%d]" % j, bar=bar, label=label, **common))
        if node.grad_outputs is None:
            continue                                   # the backward pass never reached this node (nothing behind it needs a gradient)
        y64 = tuple(widen(o) for o in node.outs)
        g64 = tuple(None if g is None else widen(g) for g in node.grad_outputs)
        if all(g is None for g in g64):
            continue
        grads = ref.vjp(a64, y64, g64)
        assert len(grads) == len(node.args), (node.name, len(grads), len(node.args))
        gin = node.aligned_grad_inputs()
        for j, (a, gd, gw) in enumerate(zip(node.args, gin, grads)):
            var = variable_of(a)
            if gd is not None:
                if gw is None:
                    raise AssertionError("#%d %s returns a gradient for argument %d, the reference has none" % (node.idx, node.name, j))
                bar, label = bar_of(node.name, ref.kind, False, gd.dtype)
                e = _compare(gd, gw, item="grad[%d]" % j, bar=bar, label=label, **common)
                rep.entries.append(e)
                if var is not None:
                    param_entries.append(e)
                if var is not None:
                    param_entries.append(e)
            elif gw is not None and var is None and node.arg_requires_grad[j] and np.abs(gw).max() > 0.0:
                # an input that required a gradient, has one in the reference, and got none from the device (a dropped consumer)
                bar, label = bar_of(node.name, ref.kind, False, a.dtype)
                m = float(np.abs(gw).max())
                rep.entries.append(Entry(err=m, ref_max=m, where=(), got=float("nan"), want=m, item="grad[%d]" % j, bar=bar,
                                         label=label + ", MISSING", **common))
            if var is not None and gw is not None and node.arg_requires_grad[j]:
                k = _vkey(var)
                c = _crop(gw, var.shape)
                expected[k] = c if k not in expected else expected[k] + c
                bar, label = bar_of(node.name, ref.kind, False, torch.float32)
                contributors.setdefault(k, []).append((node, bar, label))
    # variables: consumed, with a gradient, equal to the sum of the local gradients
    gmax = 0.0
    for name, t in variables:
        k = _vkey(t)
        if k not in expected:
            rep.unconsumed.append(name)
        elif t.grad is None:
            rep.no_grad.append(name)
        else:
            gmax = max(gmax, float(np.abs(expected[k]).max()) * abs(grad_scale))
    for name, t in variables:
        k = _vkey(t)
        if k not in expected or t.grad is None:
            continue
        nodes = contributors[k]
        bar, label = max((b, l) for _, b, l in nodes)
        e = _compare(t.grad, expected[k] * grad_scale, idx="var", name="/".join(sorted({n.name for n, _, _ in nodes})), item=name,
                     shapes=[tuple(t.shape)], plan="sum of %d node(s): %s" % (len(nodes), ",".join("#%d" % n.idx for n, _, _ in nodes)),
                     bar=bar, label=label)
        e.floor = MODEL_SCALE * gmax
        rep.var_entries.append(e)
    for e in param_entries:                           # a local parameter gradient is measured on the same model-wide scale (unscaled)
        e.floor = MODEL_SCALE * gmax / abs(grad_scale)
    rep.other_leaves = sum(k not in var_names for k in expected)      # leaves requiring grad that are no variable: data inputs of a test
    return rep


# ---- structure checks --------------------------------------------------------------------------------------------------------------
def _skey(t):
    return (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)


def producers(rec):
    """({id(tensor): (node, k)}, {storage key: (node, k)}) of every recorded output"""
    by_id, by_storage = {}, {}
    for node in rec.nodes:
        for k, o in enumerate(node.outs):
            if isinstance(o, torch.Tensor):
                by_id.setdefault(id(o), (node, k))
                by_storage.setdefault(_skey(o), (node, k))     # the FIRST producer of a storage: Fork / Mark views alias their input
    return by_id, by_storage


def cut_edges(rec):
    """[(producer class, output index, consumer class, argument index)]: a recorded tensor input that aliases a recorded output (the same
    object, or the same storage, offset, shape and strides as through ForkFn / MarkFn views or a detach()) and arrives NOT requiring grad
    although the producer's output did"""
    by_id, by_storage = producers(rec)
    cuts = []
    for node in rec.nodes:
        for j, a in enumerate(node.args):
            if not isinstance(a, torch.Tensor) or node.arg_requires_grad[j]:
                continue
            src = by_id.get(id(a)) or by_storage.get(_skey(a))
            if src is None or src[0].idx >= node.idx:
                continue
            if src[0].outs[src[1]].requires_grad:
                cuts.append((src[0].name, src[1], node.name, j))
    return cuts


def unforked_fanouts(rec):
    """[(producer class, sorted consumer classes)]: a recorded output requiring grad that is handed AS THE SAME OBJECT to more than one
    recorded node -- autograd then sums the consumers' gradients with its own add instead of ForkFn's kernel"""
    by_id, _ = producers(rec)
    users = {}
    for node in rec.nodes:
        seen = set()
        for j, a in enumerate(node.args):
            if isinstance(a, torch.Tensor) and id(a) in by_id and node.arg_requires_grad[j] and id(a) not in seen:
                seen.add(id(a))
                users.setdefault(id(a), []).append(node.name)
    return sorted((by_id[i][0].name, tuple(sorted(u))) for i, u in users.items() if len(u) > 1)


def foreign_nodes(rec, roots=None):
    """{backward-node class name: count} of every node reachable from the roots (default: the tensors backward() was called on) that is
    not the node of a recorded Function.  The walk follows next_functions only; it runs no kernel."""
    own = {n.grad_fn for n in rec.nodes if n.grad_fn is not None}
    stack = [r.grad_fn for r in (rec.roots if roots is None else roots) if r.grad_fn is not None]
    seen, found = set(), {}
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if fn not in own:
            nm = type(fn).__name__
            found[nm] = found.get(nm, 0) + 1
        stack.extend(f for f, _ in fn.next_functions)
    return found


def reached_variables(rec, roots=None):
    """the leaf tensors whose AccumulateGrad node is reachable from the roots"""
    stack = [r.grad_fn for r in (rec.roots if roots is None else roots) if r.grad_fn is not None]
    seen, leaves = set(), []
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if type(fn).__name__ == "AccumulateGrad":
            leaves.append(fn.variable)
        stack.extend(f for f, _ in fn.next_functions)
    return leaves
