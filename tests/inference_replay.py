"""Replay of a recorded TAPE-FREE forward pass, launch by launch, against float64 local references -- test infrastructure.

Under `torch.no_grad()` the nets never reach `_autograd`: they call the public entry points of `_ops` directly, in fused forms that exist
nowhere else (folded BatchNorm epilogues, `cout_valid` heads, pooled and projected second outputs, the bilinear prologue, the composed
Hallucination tail).  A whole-net bar dilutes an error of one deep or narrow layer by everything behind it.  So this module records every
call of those entry points during one forward pass -- the device's own operands and outputs -- and compares each launch with a float64
statement of that launch alone (tests/tape_replay.py does the same for the tape).

  record(K)                 context manager: shadows the public entry points of module K (the nets look them up as `K.<name>` at call time),
                            `K._lib.check` (the name of every C ABI call) and, with audit=True, `K._range_of` / `K._set_range`
  OPS                       entry point -> Op(kind, reference, feature-map operands): float64, NumPy, nothing of the package under test
  replay(rec)               per top-level launch and output: |device - reference| against the maximum of the reference, bar tape_replay.bar_of
  open_inputs(rec, inputs)  the closed-chain check: every feature-map operand equals, by snapshot, an earlier recorded output or an input
  derived_catalog(models)   the tensors the inference path derives from the variables (folded BatchNorm, padded filters, the composed tail
                            and its projections), each with its float64 formula and a counted fp32 bar
  RangeAudit                every range a split-operand launch consumed beside max |t| of the tensor it was consumed for

The only new reference code is the glue the existing references lack: the full inference epilogue around tape_replay.conv_fwd, the
bilinear prologue in front of it, the pooled second output and the projected output.  Importing this module needs no GPU.
"""
import collections
import contextlib
import inspect
import sys

import numpy as np
import torch

import conv_ref
import fp16_ref as H
import tape_ref as TR
import tape_replay as TP
import up2_fused_ref as UF

f32c, widen = TP.f32c, TP.widen
BN_EPS = 1e-3             # tf.keras.layers.BatchNormalization's default, as _layers.BN_EPS
RSQRT = 4                 # rsqrt: 2 fp32 ulps (assumed, as in tests/test_gpu_tape_f32.py), in units of 2^-24
U32 = TR.U32


# ---- float64 local references: the glue -------------------------------------------------------------------------------------------
def conv_chain(x, w, bias=None, stride=1, x2=None, x2_scale=1.0, act1=0, scale=None, shift=None, residual=None, act2=0, cout_valid=None,
               up2=False):
    """act2(affine(act1(conv(concat[up2(x), x2_scale x2], w[..., :cout_valid]) + bias)) + residual): the inference epilogue around
    tape_replay.conv_fwd.  scale / shift / residual may be wider than the stored channels (a residual read with a channel stride, constants
    of a padded head): their leading channels count."""
    xin = H.resize2x(x) if up2 else x
    (y,) = TP.conv_fwd(xin, x2, w, bias, stride, x2_scale, act1, cout_valid)
    cv = y.shape[-1]
    lead = lambda v: None if v is None else np.asarray(v)[..., :cv]      # noqa: E731
    return TR.affine_act(y, lead(scale), lead(shift), lead(residual), act2)


def projected(y, proj):
    """sum_c proj[j, c] y[..., c]"""
    return conv_ref.project(y, proj)[0]


def _conv2d(a):
    for k in ("out", "pad", "out_hw"):
        assert a[k] is None, "conv2d(%s=...) is raw-kernel plumbing, not a launch of the inference path" % k
    assert not a["w_batch_stride"]
    return (conv_chain(a["x"], a["w"], a["bias"], a["stride"], a["x2"], a["x2_scale"], a["act1"], a["scale"], a["shift"], a["residual"],
                       a["act2"], a["cout_valid"]),)


def _conv2d_up2(a):
    y = conv_chain(a["x"], a["w"], a["bias"], act1=a["act1"], scale=a["scale"], shift=a["shift"], act2=a["act2"], up2=True)
    return (y if a["proj"] is None else projected(y, a["proj"]),)


def _conv2d_maxpool2(a):
    y = conv_chain(a["x"], a["w"], a["bias"], act1=a["act1"])
    if a["proj"] is not None:
        return (projected(y, a["proj"]), H.maxpool2(y))
    return (y, H.maxpool2(y)) if a["keep_y"] else (H.maxpool2(y),)


def _conv2d_avgpool2(a):
    y = conv_chain(a["x"], a["w"], a["bias"], x2=a["x2"], act1=a["act1"])
    return (y, H.avgpool2(y))


def _alpha_blend(a):
    A, alpha = TR.alpha_blend(a["b_pred"], a["hal_bgr"], f32c(a["thr"]))
    return (A, alpha) if a["return_alpha"] else (A,)


class Op:
    """kind: the bar class of tape_replay.bar_of; ref(a) -> tuple of float64 outputs (a: operands by name, tensors widened);
    features: the operands that are feature maps (the closed-chain check); conv: a convolution (fp16 operands take the fp16 conv bar)"""

    def __init__(self, kind, ref, features, conv=False):
        self.kind, self.ref, self.features, self.conv = kind, ref, features, conv


OPS = {
    "conv2d": Op("conv", _conv2d, ("x", "x2", "residual"), True),
    "conv2d_up2": Op("conv", _conv2d_up2, ("x",), True),
    "conv2d_maxpool2": Op("conv", _conv2d_maxpool2, ("x",), True),
    "conv2d_avgpool2": Op("conv", _conv2d_avgpool2, ("x", "x2"), True),
    "affine_act": Op("bn", lambda a: (TR.affine_act(a["x"], a["scale"], a["shift"], a["residual"], a["act"]),), ("x", "residual")),
    "add": Op("glue", lambda a: (H.add(a["a"], a["b"], a["relu"]),), ("a", "b")),
    "clip": Op("glue", lambda a: (TR.clip(a["x"], f32c(a["lo"]), f32c(a["hi"])),), ("x",)),
    "vgg_preprocess": Op("glue", lambda a: (TR.vgg_preprocess(a["x"], a["out_channels"]),), ("x",)),
    "pack3": Op("glue", lambda a: (H.pack3(a["srcs"], a["out_channels"] or 3 * len(a["srcs"])),), ("srcs",)),
    "alpha_blend": Op("glue", _alpha_blend, ("b_pred", "hal_bgr")),
    "apply_rf": Op("crf", lambda a: TP.apply_rf_fwd(a["x"], a["rf"]), ("x", "rf")),
    "lin_frontend": Op("glue", lambda a: (H.lin_frontend(a["img"], a["channels"]),), ("img",)),
    "soft_hist": Op("glue", lambda a: (TR.soft_hist(a["img"], a["max_bin"]),), ("img",)),
    "invcrf_decode": Op("crf", lambda a: (TR.invcrf_decode(a["feat"], a["wfc"], a["bfc"], a["table"]),), ("feat",)),
    "increase": Op("crf", lambda a: (TR.increase(a["rf"]),), ("rf",)),
    "maxpool3s2": Op("glue", lambda a: (H.maxpool3s2(a["x"]),), ("x",)),
    "maxpool2": Op("glue", lambda a: (H.maxpool2(a["x"]),), ("x",)),
    "global_avg_pool": Op("glue", lambda a: (H.gap(a["x"]),), ("x",)),
    "avgpool2": Op("glue", lambda a: (H.avgpool2(a["x"]),), ("x",)),
    "resize2x": Op("glue", lambda a: (H.resize2x(a["x"]),), ("x",)),
    "reverse3": Op("glue", lambda a: (TR.reverse3(a["x"]),), ("x",)),
    "fork": Op("glue", lambda a: (a["x"],) * a["n"], ("x",)),
    "mark": Op("glue", lambda a: (a["x"],), ("x",)),
}
POOLED = ("conv2d_maxpool2", "conv2d_avgpool2")
# Measured bar: the composed Hallucination tail in native fp16 -- conv2d on fp16 u1 and d1 with a `cout_valid` head,
# folded norm2 and relu.  The three outputs are relu(sc (W_u u1 + W_d d1 / 255 + b) + sh): the terms cancel and relu keeps the small
# positive remainder, so the maximum of the output lies far below the magnitudes the fp16 roundings of the packed filter act on.  Worst
# measured distance 9.272e-3 of the reference's maximum ((2, 32, 96), seed 123); the bar is the next power of two above twice that.
FP16_TAIL_BAR = 2.0 ** -5


def conv_terms(a):
    """max over the elements of sum |terms| of a conv2d launch: |scale| (sum |x| |w| + |bias|) + |shift| + |residual| -- the magnitude the
    roundings of the operands act on (report only)"""
    ab = lambda v: None if v is None else np.abs(v)      # noqa: E731
    (y,) = TP.conv_fwd(ab(a["x"]), ab(a["x2"]), ab(a["w"]), ab(a["bias"]), a["stride"], a["x2_scale"], 0, a["cout_valid"])
    cv = y.shape[-1]
    lead = lambda v: None if v is None else np.asarray(v)[..., :cv]      # noqa: E731
    return float(TR.affine_pre(y, lead(a["scale"]), lead(a["shift"]), lead(a["residual"]), absolute=True).max())


def is_fp16_tail(launch):
    a = launch.a
    return (launch.op == "conv2d" and launch.dtype == torch.float16 and a["cout_valid"] is not None and a["cout_valid"] < a["w"].shape[3]
            and a["x2"] is not None and a["shift"] is not None and a["act2"] == TP.ACT_RELU)


# ---- the recorder ------------------------------------------------------------------------------------------------------------------
def _is_t(v):
    return isinstance(v, torch.Tensor)


def _snap(v):
    if _is_t(v):
        with torch.no_grad():
            return v.detach().clone()
    if isinstance(v, (list, tuple)) and v and all(_is_t(t) for t in v):
        return [_snap(t) for t in v]
    return v


def _tensors(v):
    return [v] if _is_t(v) else ([t for t in v if _is_t(t)] if isinstance(v, (list, tuple)) else [])


class Launch:
    """one call of a recorded entry point: op, live (operands by name as they were handed over), a (the same with every tensor
    snapshotted AFTER the call), outs (flat tuple, None entries kept), form ("single" | "tuple" | "none"), prec (K.PRECISION), dtype
    (of the first feature-map operand), plan / projected (report only), children (recorded calls made inside), abi (C ABI entry points
    called inside, children's included)"""

    def __init__(self, idx, op, live, prec):
        self.idx, self.op, self.live, self.prec = idx, op, live, prec
        self.a, self.outs, self.form, self.children, self.abi, self.plan, self.projected = None, (), "none", [], [], None, 0
        first = next((t for n in OPS[op].features for t in _tensors(live.get(n))), None)
        self.dtype = None if first is None else first.dtype

    def finish(self, out):
        self.form = "none" if out is None else ("tuple" if isinstance(out, tuple) else "single")
        self.outs = () if out is None else (tuple(out) if isinstance(out, tuple) else (out,))
        self.a = collections.OrderedDict((k, _snap(v)) for k, v in self.live.items())

    def features(self, snapshots=True):
        src = self.a if snapshots else self.live
        return [(n, t) for n in OPS[self.op].features for t in _tensors(src.get(n))]

    def shapes(self):
        return [tuple(t.shape) for _, t in self.features()]

    def walk(self):
        yield self
        for c in self.children:
            yield from c.walk()

    def __repr__(self):
        return "#%d %s %s" % (self.idx, self.op, self.shapes())


class Recording:
    def __init__(self, module):
        self.module = module
        self.launches = []        # top level, in call order
        self.outside = []         # C ABI entry points called outside every recorded launch
        self.audit = None
        self.count = 0

    def of(self, op):
        return [l for l in self.launches if l.op == op]

    def all(self):
        for l in self.launches:
            yield from l.walk()

    def abi_names(self):
        return {n for l in self.launches for n in l.abi}


def _plan(K, launch):
    """the kernel family of a convolution launch, asked from the library; for the report only"""
    a = launch.live
    try:
        x, w = a["x"], a["w"]
        if x.dtype != torch.float32:
            return "fp16"
        shape = tuple(x.shape)
        if launch.op == "conv2d_up2":
            shape = (shape[0], 2 * shape[1], 2 * shape[2], shape[3])
        x2 = a.get("x2")
        return K.conv2d_plan(shape, tuple(w.shape), 0 if x2 is None else x2.shape[3], a.get("stride", 1), a.get("x2_scale", 1.0),
                             a.get("residual") is not None, a.get("cout_valid"))
    except Exception:
        return "?"


@contextlib.contextmanager
def record(K, names=None, audit=False):
    """with record(K) as rec: <tape-free forward>.  names: the entry points to shadow (default: every name of OPS the module has).  The
    product code is untouched: each name is shadowed on the module and restored on exit.  audit=True: rec.audit is a RangeAudit of the pass."""
    rec = Recording(K)
    names = [n for n in OPS if hasattr(K, n)] if names is None else list(names)
    stack, saved = [], []
    lib = getattr(K, "_lib", None)

    def wrap(name, orig):
        sig = inspect.signature(orig)

        def recorded(*args, **kw):
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            launch = Launch(rec.count, name, collections.OrderedDict(ba.arguments), getattr(K, "PRECISION", None))
            rec.count += 1
            before = getattr(K, "PROJECTED_LAUNCHES", [0])[0]
            stack.append(launch)
            try:
                out = orig(*args, **kw)
            finally:
                stack.pop()
            launch.finish(out)
            launch.projected = getattr(K, "PROJECTED_LAUNCHES", [0])[0] - before
            if OPS[name].conv and hasattr(K, "conv2d_plan"):
                launch.plan = _plan(K, launch)
            (stack[-1].children if stack else rec.launches).append(launch)
            return out
        recorded.__name__ = name
        return recorded

    def patch(obj, name, new):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)
    try:
        for n in names:
            patch(K, n, wrap(n, getattr(K, n)))
        if lib is not None and hasattr(lib, "check"):
            check = lib.check

            def checked(rc, name, *a, **kw):
                for l in stack:
                    l.abi.append(name)
                if not stack:
                    rec.outside.append(name)
                return check(rc, name, *a, **kw)
            patch(lib, "check", checked)
        if audit:
            rec.audit = RangeAudit(K, stack)
            rec.audit.install(patch)
        yield rec
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)


# ---- the replay ------------------------------------------------------------------------------------------------------------------------
def bar_of(launch, out, item):
    """(bar, label): the project's op-level bars from where they live -- tape_replay.bar_of (fp32 feature maps 1e-5, the CRF head 2e-4,
    fp16 convolutions, one fp16 ulp for an fp16 elementwise result) and up2_fused_ref.TOL for a projected output"""
    op = OPS[launch.op]
    if op.conv and launch.dtype == torch.float16:
        if launch.op == "conv2d" and is_fp16_tail(launch):
            return FP16_TAIL_BAR, "fp16 composed tail (measured)"
        return TP.bar_of("Conv2dHFn", op.kind, True, out.dtype)
    if item == "proj":
        return UF.TOL, "fp32 projected output"
    return TP.bar_of(launch.op, op.kind, True, out.dtype)


def _items(launch):
    if launch.op in ("conv2d_up2", "conv2d_maxpool2") and launch.a.get("proj") is not None:
        return ["proj", "pooled"][:len(launch.outs)]
    if launch.op in POOLED:
        return ["y", "pooled"] if len(launch.outs) == 2 else ["pooled"]
    return ["out[%d]" % j for j in range(len(launch.outs))]


class Report(TP.Report):
    def assert_ok(self, leave=None):
        bad = [e for e in self.failures() if leave is None or not leave(e)]
        if bad:
            raise AssertionError("inference replay: %d of %d comparisons outside their bar\n%s" % (
                len(bad), len(self.entries) + len(self.var_entries), "\n".join(e.line() for e in bad)))

    def failed(self):
        return {(e.idx, e.item) for e in self.entries if not e.ok}


def replay(rec):
    """Compare every output of every TOP-LEVEL launch with its float64 local reference, fed the launch's own operands widened to float64
    (an fp16 operand with the values the fp16 tensor holds).  Per element against the maximum of the reference; no element is excluded.
    A launch that returned None (a form the planned kernel cannot take: the caller falls back) has nothing to compare."""
    rep = Report()
    for l in rec.launches:
        if l.op not in OPS:
            raise KeyError("no float64 reference registered for %s" % l.op)
        if l.form == "none":
            continue
        a64 = {k: (widen(v) if _is_t(v) else [widen(t) for t in v] if isinstance(v, list) and v and _is_t(v[0]) else v) for k, v in l.a.items()}
        want = OPS[l.op].ref(a64)
        assert len(want) == len(l.outs), (l, len(want), len(l.outs))
        for o, wv, item in zip(l.outs, want, _items(l)):
            if o is None:
                continue
            bar, label = bar_of(l, o, item)
            rep.entries.append(TP._compare(o, wv, idx=l.idx, name=l.op, item=item, shapes=l.shapes(), bar=bar, label=label,
                                           plan="%s/%s" % (l.plan or "-", l.prec)))
    return rep


def _same(t, k):
    return t.shape == k.shape and t.dtype == k.dtype and t.device == k.device and bool(torch.equal(t, k))


def open_inputs(rec, inputs):
    """[(launch, operand name)]: feature-map operands of top-level launches that equal, by snapshot, neither an earlier recorded output
    nor one of `inputs` -- an op that slipped between two recorded ops leaves one"""
    known = list(inputs)
    gaps = []
    for l in rec.launches:
        for name, t in l.features():
            if not any(_same(t, k) for k in reversed(known)):
                gaps.append((l, name))
        known.extend(o for o in l.outs if _is_t(o))
    return gaps


# ---- derived operands against the variables ----------------------------------------------------------------------------------------------
class Derived:
    """one tensor the inference path derives from the variables: name, the live tensor, its float64 formula `want`, the counted bar
    `allow` (an array, per element; None: bit for bit) and the count written beside it"""

    def __init__(self, name, tensor, want, allow, count):
        self.name, self.tensor, self.want, self.allow, self.count = name, tensor, np.asarray(want, dtype=np.float64), allow, count

    def compare(self, t=None):
        got = widen(self.tensor if t is None else t)
        assert got.shape == self.want.shape, (self.name, got.shape, self.want.shape)
        d = np.abs(got - self.want)
        d = np.where(np.isfinite(d), d, np.inf)
        allow = np.zeros(d.shape) if self.allow is None else np.broadcast_to(self.allow, d.shape)
        over = d - allow
        k = int(np.argmax(over))
        return DerivedEntry(self.name, self.count, float(d.reshape(-1)[k]), float(allow.reshape(-1)[k]), bool((d <= allow).all()),
                            tuple(int(i) for i in np.unravel_index(k, d.shape)), float(got.reshape(-1)[k]), float(self.want.reshape(-1)[k]))


class DerivedEntry:
    def __init__(self, name, count, err, allow, ok, where, got, want):
        self.name, self.count, self.err, self.allow, self.ok, self.where, self.got, self.want = name, count, err, allow, ok, where, got, want

    def line(self):
        return "%s %-44s |err| %.3e allowed %.3e (%s) at %s got %.9g want %.9g" % (
            "ok  " if self.ok else "FAIL", self.name, self.err, self.allow, self.count, self.where, self.got, self.want)


def _walk(layer, prefix=""):
    yield prefix.rstrip("."), layer
    for name, child in layer._children:
        yield from _walk(child, prefix + name + ".")


def _v(t):
    return widen(t)


def folded_formula(bn):
    """(scale, shift, |terms| of shift) in float64 from the variables (eps exact: its cast to fp32 is counted in the bar)"""
    g, b, m, v = (_v(t) for t in (bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance))
    scale = g / np.sqrt(v + BN_EPS)
    return scale, b - m * scale, np.abs(b) + np.abs(m * scale)


def tail_formula(model, c_skip=64):
    """(wc [128, 3], |terms| of wc, bc [3], |terms| of bc) of the composed tail s1 -> conv2, the 1 / 255 on the skip rows of W1"""
    k1, b1, k2, b2 = (_v(t) for t in (model.s1.conv1.kernel, model.s1.conv1.bias, model.conv2.kernel, model.conv2.bias))
    w1 = k1.reshape(k1.shape[2], k1.shape[3]).copy()
    w1[w1.shape[0] - c_skip:] *= 1.0 / 255
    w2 = k2.reshape(k2.shape[2], k2.shape[3])
    return w1 @ w2, np.abs(w1) @ np.abs(w2), b1 @ w2 + b2, np.abs(b1) @ np.abs(w2) + np.abs(b2)


def _key(t):
    return (t.data_ptr(), tuple(t.shape))          # (up_filter is a leading view of wc: the same address)


def derived_catalog(models):
    """{(data_ptr, shape): Derived} of every derived tensor the models hold after a tape-free pass (their per-version caches), found by walking each
    model once.  models: {prefix: model}.  The counts k (units of 2^-24 on the sum of the magnitudes of an element's terms):
      scale  = gamma * rsqrt(var + eps)      k = 3 + RSQRT: the cast of eps, the sum, rsqrt's units, the product
      shift  = beta - mean * scale           k = 5 + RSQRT: scale's, the product, the difference
      wc, bc                                 k = 1: composed in float64, rounded to fp32 once
      maps   = wc * sc                       k = 5 + RSQRT: wc's, scale's, the product
      const  = sc * bc + sh                  k = 7 + RSQRT on |sc| sum|bc terms|, shift's on its own terms, one more for the sum"""
    cat = {}

    def put(d):
        cat[_key(d.tensor)] = d
    for prefix, model in models.items():
        for path, layer in _walk(model, prefix + "." if prefix else ""):
            folded = getattr(layer, "_folded", None)
            if folded is not None and hasattr(layer, "moving_variance"):
                scale, shift, mags = folded_formula(layer)
                put(Derived(path + ".folded.scale", folded[1], scale, (3 + RSQRT) * U32 * np.abs(scale), "k = 3 + RSQRT"))
                put(Derived(path + ".folded.shift", folded[2], shift, (5 + RSQRT) * U32 * mags, "k = 5 + RSQRT"))
            padded = getattr(layer, "_padded", None)
            if padded is not None and hasattr(layer, "kernel"):
                k = _v(layer.kernel)
                want = np.zeros(tuple(padded[1].shape))
                want[:, :, :k.shape[2], :k.shape[3]] = k
                put(Derived(path + ".kernel_padded", padded[1], want, None, "bit for bit"))
            tail = getattr(layer, "_tail", None)
            if tail is not None and hasattr(layer, "s1"):
                wc, wc_mag, bc, bc_mag = tail_formula(layer, tail[0][4])
                want, mag = np.zeros(tuple(tail[1].shape)), np.zeros(tuple(tail[1].shape))
                want[0, 0, :, :3], mag[0, 0, :, :3] = wc, wc_mag
                put(Derived(path + "._tail_filter.wc", tail[1], want, U32 * mag, "k = 1"))
                put(Derived(path + "._tail_filter.bc", tail[2], bc, U32 * bc_mag, "k = 1"))
                proj = getattr(layer, "_tail_proj", None)
                if proj is not None:
                    sc, sh, sh_mag = (v[:3] for v in folded_formula(layer.norm2))
                    m, m_mag = (wc * sc).T, (wc_mag * np.abs(sc)).T                       # [3, 128]
                    d = proj[1]
                    put(Derived(path + "._tail_projection.up_map", d["up_map"], m[:, :64], (5 + RSQRT) * U32 * m_mag[:, :64], "k = 5 + RSQRT"))
                    put(Derived(path + "._tail_projection.skip_map", d["skip_map"], m[:, 64:], (5 + RSQRT) * U32 * m_mag[:, 64:], "k = 5 + RSQRT"))
                    put(Derived(path + "._tail_projection.const", d["const"], sc * bc + sh,
                                U32 * ((7 + RSQRT) * np.abs(sc) * bc_mag + (5 + RSQRT) * sh_mag + np.abs(sc * bc + sh)), "k = 7 + RSQRT"))
                    put(Derived(path + "._tail_projection.up_filter", d["up_filter"], want[:, :, :64, :], U32 * mag[:, :, :64, :], "k = 1"))
    return cat


PARAMETER_OPERANDS = ("w", "bias", "scale", "shift", "proj")


def derived_report(rec, models):
    """(entries, unresolved): every parameter operand of every recorded launch (nested ones included) is a variable of the models or one
    of the catalogued derived tensors; each derived tensor that a launch consumed is compared ONCE, as the launch's snapshot of it, with
    its float64 formula.  unresolved: [(launch, operand name)] that are neither."""
    cat = derived_catalog(models)
    variables = {t.data_ptr() for m in models.values() for _, t, _ in m.named_weights()}
    entries, unresolved, seen = [], [], set()
    for l in rec.all():
        for name in PARAMETER_OPERANDS:
            t = l.live.get(name)
            if not _is_t(t):
                continue
            d = cat.get(_key(t))
            if d is not None and d.tensor is t:
                if _key(t) not in seen:
                    seen.add(_key(t))
                    entries.append(d.compare(l.a[name]))
            elif t.data_ptr() not in variables:
                unresolved.append((l, name))
    return entries, unresolved


# ---- range audit -------------------------------------------------------------------------------------------------------------------------
class Consumed:
    """one consumption of a range: the function that asked (`_conv2d_raw`, `conv2d_dgrad`, ...), the tensor's shape, kind ("slot": written
    by a kernel, "host": a host bound turned into a constant slot), exact (the slot was written for this very tensor: it must EQUAL the
    maximum), and after RangeAudit.finish(): consumed, actual (floats)"""

    def __init__(self, who, shape, kind, exact, bound, consumed, actual):
        self.who, self.shape, self.kind, self.exact, self.bound, self.consumed, self.actual = who, shape, kind, exact, bound, consumed, actual

    @property
    def sound(self):
        return self.consumed >= self.actual

    @property
    def ok(self):
        return self.sound and (not self.exact or self.consumed == self.actual)

    def line(self):
        return "%s %-22s %-5s%s %-22s consumed %.9g actual max %.9g" % ("ok  " if self.ok else "FAIL", self.who, self.kind,
                                                                         " (exact)" if self.exact else "", self.shape, self.consumed, self.actual)


class RangeAudit:
    """Shadows K._range_of and K._set_range.  For every tensor whose range is consumed, max |t| is queued on the same stream beside a copy
    of the slot that was returned; finish() synchronises once and turns both into floats."""

    def __init__(self, K, stack=None):
        self.K, self.stack, self.items, self.owner, self.misses0 = K, stack if stack is not None else [], [], {}, collections.Counter(K.RANGE_MISSES)

    def install(self, patch):
        K, range_of, set_range = self.K, self.K._range_of, self.K._set_range

        def audited_range_of(t):
            slot = range_of(t)
            if slot is not None and _is_t(t):
                s, b = K._record(t)
                # a host bound travels as a constant slot: made here (s is None), or re-attached as a slot by a backward node that kept it
                host = s is None or any(s is c for c in getattr(K, "_CONST_SLOTS", {}).values())
                own = self.owner.get(slot.data_ptr())
                with torch.no_grad():
                    self.items.append(Consumed(sys._getframe(1).f_code.co_name, tuple(t.shape), "host" if host else "slot",
                                               not host and own is not None and own[1] is t and own[2], b, slot.detach().clone(),
                                               t.detach().abs().max().float()))
            return slot

        def audited_set_range(t, slot, bound=None):
            if slot is not None and slot.data_ptr() not in self.owner:
                who = sys._getframe(1).f_code.co_name
                top = self.stack[-1] if self.stack else None
                pooled = top is not None and top.op in POOLED and _is_t(top.live.get("x")) and t.dim() == 4 and 2 * t.shape[1] == top.live["x"].shape[1]
                # (slot kept: its slab stays allocated, so no later slot of the pass takes its address; t kept: identity)
                self.owner[slot.data_ptr()] = (slot, t, who != "_carry_range" and not pooled)
            return set_range(t, slot, bound)
        patch(K, "_range_of", audited_range_of)
        patch(K, "_set_range", audited_set_range)

    def finish(self):
        if self.items and _is_t(self.items[0].consumed) and self.items[0].consumed.is_cuda:
            torch.cuda.synchronize()
        for c in self.items:
            if _is_t(c.consumed):
                c.consumed, c.actual = float(c.consumed.item()), float(c.actual.item())
        self.owner = {}
        return self

    def failures(self):
        return [c for c in self.items if not c.ok]

    def misses(self):
        """the growth of K.RANGE_MISSES since the audit began"""
        return collections.Counter(self.K.RANGE_MISSES) - self.misses0

    def looseness(self):
        """{(consumer, kind): (worst consumed / actual, count)}; a consumption of an all-zero tensor is left out of the ratio"""
        out = {}
        for c in self.items:
            r = c.consumed / c.actual if c.actual > 0 else 1.0
            w, n = out.get((c.who, c.kind), (0.0, 0))
            out[(c.who, c.kind)] = (max(w, r), n + 1)
        return out

    def summary(self):
        return "\n".join("range %-22s %-5s %4d consumption(s), worst consumed / actual %.4g" % (k[0], k[1], v[1], v[0])
                         for k, v in sorted(self.looseness().items()))

    def assert_sound(self):
        bad = self.failures()
        if bad:
            raise AssertionError("range audit: %d of %d consumptions wrong\n%s" % (len(bad), len(self.items), "\n".join(c.line() for c in bad)))


@contextlib.contextmanager
def audit_ranges(K):
    """with audit_ranges(K) as aud: <forward and backward>; aud.finish() afterwards.  The audit alone, without the launch recorder."""
    saved = []

    def patch(obj, name, new):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)
    aud = RangeAudit(K)
    try:
        aud.install(patch)
        yield aud
    finally:
        for obj, name, old in reversed(saved):
            setattr(obj, name, old)
