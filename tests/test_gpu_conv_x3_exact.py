"""The split-operand fp32 convolution kernels -- conv_x3_kernel, conv_x3_wide_kernel, conv_x3_1x1_kernel (csrc/conv_x3.hip) and conv_x3n_kernel
(csrc/conv_x3n.hip), forward and input gradient -- against the float64 model of tests/conv_ref.py (conv_split), EXACTLY and element
by element (DESIGN.md sections 4.5 and 4.6).

The model restates what the kernels compute, not the ideal convolution: x 2^T = xh + xl 2^-11 (T from the range slot), w 2^S =
wh + wl, and acc = sum xh wh + sum xl (wh 2^-11) + sum xh wl -- the xl wl 2^-11 term is dropped.  Three operand modes:
  int     x integers in [-2, 2] (slot 2.0: T = 9), w in {-1, 0, 1} (S = 13): both low planes are empty -- layout, taps, chunks, edges;
  fx      x = (k + j 2^-11) 2^-7 under the slot 8.0 (T = 7): xh = k, xl = j -- the cross term xl ws alone;
  fw      w = q / 2 + r 2^-13: wh = 4096 q, ws = 2 q, wl = r -- the cross term xh wl alone;
  fxw     both: the dropped term is non-zero and the reference differs from the true convolution on most outputs.
Every case asserts on the reference, BEFORE the kernel is called, that the sum of absolute terms of every output is below 2^24 units
of the terms' common lsb: the fp32 accumulator then holds every partial sum exactly, in any order (MFMA order, chunks, phases, taps).
The epilogue is conv_ref.epilogue: one fp32 rounding per step; biases, shifts and residuals are integers, scales powers of two (an
FMA-contracted affine gives the same bits), projection rows small integers (their sums are asserted exact as well).

Every comparison is whole-tensor equality of bit patterns with -0 mapped to +0; a difference names the first differing index, its
16 x 16 tile (or 128-pixel block) and got / want.  Every output -- y, the pooled and projected tensors, dx -- and the range slot sit
between guard words of a NaN pattern.  The slot must hold the bits of max |y_ref| (or a larger value it held before).  The C ABI is
called through shdr._lib, as tests/test_gpu_abi.py does; test_wrapper_* go through shdr._ops.conv2d(out=...) / conv2d_dgrad.

Which instantiation a case runs is DERIVED FROM THE DISPATCH CODE (x3_forward / launch_x3 / launch_x3_1x1 in conv_x3.hip, dispatch_ct /
shdr_conv2d_fwd_x3n_ranged_f32 in conv_x3n.hip, dgrad_geom in conv_plan.hip), restated in `instance()` below; the plan itself is asked
from the library per case (shdr_conv2d_plan_f32) and asserted.  The plans are forced with the existing switches only."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import conv_ref as C
from test_gpu_wgrad_f32_exact import FINE_PAIRS, GUARD, SENT32, P, guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

LIMIT = 2.0 ** 24
E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5
PLAN = {0: "direct", 1: "mfma", 2: "fused", 3: "planes", 4: "x3", 5: "x3n"}
S8 = 2.0 ** -8
SIZES = [(1, 1), (15, 16), (16, 17), (17, 15), (33, 16), (16, 33), (1, 33), (33, 1), (15, 15), (17, 33)]      # from {1, 15, 16, 17, 33}^2


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# operand recipes (pure NumPy: tests/test_conv_ref.py pins the planes they promise)
# ---------------------------------------------------------------------------------------------------------------------------------
def seed_of(name):
    return zlib.crc32(name.encode())


def thin_out(rng, a, keep):
    return a if keep >= 1.0 else a * (rng.random(a.shape) < keep)


def int_x(rng, shape, keep=1.0):
    """(x, slot bound): integers in [-2, 2], one element pinned to 2 so that the measured range IS the declared bound 2.0"""
    x = thin_out(rng, rng.integers(-2, 3, size=shape).astype(np.float64), keep)
    x.reshape(-1)[int(rng.integers(0, x.size))] = 2.0
    return x, 2.0


def fine_x(rng, shape, keep=1.0, kmax=2):
    """(x, slot bound 8.0, k, j): x = (k + j 2^-11) 2^-7, which the split takes apart into xh = k, xl = j"""
    pairs = FINE_PAIRS[np.abs(FINE_PAIRS[:, 0]) <= kmax]
    kj = pairs[rng.integers(0, len(pairs), size=shape)]
    k, j = thin_out(rng, kj[..., 0], keep), kj[..., 1]
    j = np.where(k == 0, 0.0, j)
    return np.ldexp(k + np.ldexp(j, -11), -7), 8.0, k, j


def int_w(rng, shape, keep=1.0, cols=None):
    """w in {-1, 0, 1} with w[0, 0, 0, 0] = 1 (S = 13): wh = 8192 w, ws = 4 w, wl = 0; columns >= cols are zero (a padded head)"""
    w = thin_out(rng, rng.integers(-1, 2, size=shape).astype(np.float64), keep)
    w[0, 0, 0, 0] = 1.0
    if cols is not None:
        w[..., cols:] = 0.0
    return w


def fine_w(rng, shape, keep=1.0, cols=None):
    """(w, q, r): w = q / 2 + r 2^-13, r = 0 where q = 0, w[0, 0, 0, 0] = 1 (S = 13): wh = 4096 q, ws = 2 q, wl = r"""
    q = thin_out(rng, rng.integers(-1, 2, size=shape).astype(np.float64), keep)
    r = np.where(q == 0, 0.0, rng.integers(-1, 2, size=shape).astype(np.float64))
    q[0, 0, 0, 0], r[0, 0, 0, 0] = 2.0, 0.0
    if cols is not None:
        q[..., cols:] = 0.0
        r[..., cols:] = 0.0
    return q / 2 + np.ldexp(r, -13), q, r


def operands(name, n, h, w, c1, c2, cout, k, mode, x2s=1.0, keep=1.0, kmax=2, cols=None):
    """(x, x_bound, x2, x2_bound, w) of a case.  The second source holds integers m in [-2, 2] times 1 / x2_scale (a power of two) --
    next to a fine first source m 2^-8 / x2_scale under the same slot 8.0, so that both sources' high planes are small integers (ONE T
    serves both sources: a second source that filled its range would dwarf the fine terms and break the precondition)."""
    rng = np.random.default_rng(seed_of(name))
    fine = mode in ("fx", "fxw")
    if fine:
        x, xb, _, _ = fine_x(rng, (n, h, w, c1), keep, kmax)
    else:
        x, xb = int_x(rng, (n, h, w, c1), keep)
    x2 = x2b = None
    if c2:
        x2, x2b = int_x(rng, (n, h, w, c2), keep)
        x2, x2b = (np.ldexp(x2, -8) / x2s, 8.0) if fine else (x2 / x2s, x2b / x2s)
    shape = (k, k, c1 + c2, cout)
    wt = fine_w(rng, shape, keep, cols)[0] if mode in ("fw", "fxw") else int_w(rng, shape, keep, cols)
    return x, xb, x2, x2b, wt


EPILOGUES = ("plain", "relu", "lrelu", "affine", "res", "act2", "nobias")


def epilogue_operands(name, epi, cv, out_shape, res_pad=8):
    """(bias, act1, scale, shift, residual, act2): integers and powers of two; residual [N, Ho, Wo, cv + res_pad]"""
    rng = np.random.default_rng(seed_of(name) ^ 0x5EED)
    bias = None if epi == "nobias" else rng.integers(-3, 4, size=cv).astype(np.float64)
    act1 = {"relu": C.ACT_RELU, "lrelu": C.ACT_LRELU, "affine": C.ACT_LRELU, "res": C.ACT_NONE, "act2": C.ACT_LRELU}.get(epi, C.ACT_NONE)
    scale = shift = res = None
    act2 = C.ACT_NONE
    if epi in ("affine", "res", "act2"):
        scale = np.ldexp(1.0, rng.integers(-1, 3, size=cv))
        shift = rng.integers(-3, 4, size=cv).astype(np.float64)
    if epi == "res":
        res = rng.integers(-4, 5, size=tuple(out_shape[:3]) + (cv + res_pad,)).astype(np.float64)
        act2 = C.ACT_RELU
    if epi == "act2":
        act2 = C.ACT_RELU
    return bias, act1, scale, shift, res, act2


# ---------------------------------------------------------------------------------------------------------------------------------
# device helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "operand not exact in fp32"
    return torch.from_numpy(a.astype(np.float32)).cuda()


def slot_of(value):
    return torch.from_numpy(np.array([value], dtype=np.float32)).cuda()


def bits32(v):
    return int(np.asarray(v, dtype=np.float32).reshape(-1).view(np.uint32)[0])


def guarded_f32(shape):
    numel = int(np.prod(shape))
    buf, v = guarded(numel)
    return buf, v.view(torch.float32).view(tuple(shape)), numel


def locate(i, where):
    if where == "pixels":                                               # conv_x3_1x1_kernel: blocks of 128 consecutive output pixels
        return "block %d (pixel %d of it)" % (i[0] // 128, i[0] % 128)
    if len(i) == 4:
        return "image %d, tile (%d, %d), pixel (%d, %d) of it" % (i[0], i[1] // 16, i[2] // 16, i[1] % 16, i[2] % 16)
    return ""


def same(got, want, what, where="tiles"):
    """bit equality with -0 mapped to +0; a difference names the first differing index, its tile or block, and got / want"""
    got = np.ascontiguousarray(got, dtype=np.float32) + np.float32(0.0)
    want = np.ascontiguousarray(want, dtype=np.float32) + np.float32(0.0)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        i = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        j = (i[0] * got.shape[1] * got.shape[2] + i[1] * got.shape[2] + i[2],) if where == "pixels" else i
        raise AssertionError("%s: %d of %d elements differ; first at %s, %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.size, i, locate(j, where), float(got[i]), float(want[i])))


class Slot:
    """a range slot between guards, holding `preset` (0 or a larger bound that must survive)"""

    def __init__(self, preset=0.0):
        self.buf, v = guarded(4)
        self.view = v.view(torch.float32)[0:1]
        self.view.fill_(preset)
        self.preset = preset

    def check(self, ymax, what):
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy().view(np.uint32)
        assert (raw[:GUARD] == SENT32).all() and (raw[GUARD + 1:] == SENT32).all(), what + ": words around the range slot were written"
        want = max(bits32(ymax), bits32(self.preset))
        assert int(raw[GUARD]) == want, "%s: range slot holds %r, want the bits of max |y_ref| = %r (preset %r)" % (
            what, float(raw[GUARD:GUARD + 1].view(np.float32)[0]), float(np.float32(ymax)), self.preset)


def wide_3x3(o, up):
    """the rule of x3_forward for the 128-cout blocks: stride 1, Cout % 128 == 0, Cout >= the cout threshold (128 with the prologue in the
    kernel, else 512; SHDR_X3_WIDE_MIN_COUT), no projected output, 16 x 16 tiles x Cout / 128 >= the block threshold (256;
    SHDR_X3_WIDE_MIN_BLOCKS), and no SHDR_X3_SLICED"""
    env, cout = o["env"], o["cout"]
    h, w = (2 * o["h"], 2 * o["w"]) if o.get("up") else (o["h"], o["w"])
    blocks = o["n"] * (-(-h // 16)) * (-(-w // 16)) * (cout // 128)
    return (o["k"] == 3 and o["stride"] == 1 and cout % 128 == 0 and cout >= int(env.get("SHDR_X3_WIDE_MIN_COUT", 128 if up else 512))
            and not o.get("proj") and blocks >= int(env.get("SHDR_X3_WIDE_MIN_BLOCKS", 256)) and "SHDR_X3_SLICED" not in env)


def instance(o):
    """the kernel instantiation the dispatch code runs for a case (see the module docstring).  It labels failure messages and the
    case tables of DESIGN.md sections 4.5 and 4.6; the library exports the plan, not the instantiation, so only the 128-cout blocks are
    asserted, by kernel name (test_wide_kernel_names)."""
    k, c1, c2, cout = o["k"], o["c1"], o["c2"], o["cout"]
    env = o["env"]
    if o["plan"] == "x3n":
        ct = 32 if c2 else (8 if c1 <= 8 else (16 if c1 <= 16 else 32))
        if cout == 64:
            return "conv_x3n_kernel<3, 8, 4, false, false>"
        return "conv_x3n_kernel<%d, %d, %d, %s, %s>" % (k, ct, cout // 16, "true" if c2 else "false", "true" if o.get("tanh") else "false")
    if o["plan"] != "x3":
        return "plan " + o["plan"]
    look = int(env.get("SHDR_X3_LOOK", 2))
    if k == 7:
        return "conv_x3_kernel<false, 4, 4, true, 1>"
    if k == 1:
        wide = cout % 128 == 0 and not o.get("pool") and not o.get("proj") and "SHDR_X3_1X1_SLICED" not in env
        return "conv_x3_1x1_kernel<%d>" % (4 if cout % 256 == 0 else 2) if wide else "conv_x3_kernel<false, 1, 1, false, %d>" % min(look, 1)
    up = bool(o.get("up")) and (cout <= 256 or "SHDR_X3_UP_ALWAYS" in env)
    if wide_3x3(o, up):
        return "%sconv_x3_wide_kernel<%s>" % ("resize2x_kernel + " if o.get("up") and not up else "", "true" if up else "false")
    return "%sconv_x3_kernel<%s, 3, 3, false, %d>" % ("resize2x_kernel + " if o.get("up") and not up else "", "true" if up else "false", look)


# ---------------------------------------------------------------------------------------------------------------------------------
# the forward runner
# ---------------------------------------------------------------------------------------------------------------------------------
def case(name, plan, n, h, w, c1, c2, cout, k, stride=1, mode="int", epi="plain", **o):
    o.update(name=name, plan=plan, n=n, h=h, w=w, c1=c1, c2=c2, cout=cout, k=k, stride=stride, mode=mode, epi=epi)
    o.setdefault("env", {})
    o.setdefault("x2s", 1.0)
    return pytest.param(o, id=name)


def reference(o, bounds=None):
    """everything of a case that needs no device: operands, the model, the precondition, the expected outputs.  bounds = (x1's, x2's)
    replaces the slot contents the operands come with (test_unusual_slot_contents)"""
    name, n, h, w, c1, c2, cout, k, stride = (o[f] for f in ("name", "n", "h", "w", "c1", "c2", "cout", "k", "stride"))
    cv = o.get("cv") or cout
    x, xb, x2, x2b, wt = operands(name, n, h, w, c1, c2, cout, k, o["mode"], o["x2s"], o.get("keep", 1.0), o.get("kmax", 2),
                                  cv if cv != cout else None)
    if bounds is not None:
        xb, x2b = bounds
    xin = x
    if o.get("up"):                                                      # the descriptor's H, W are the up-sampled ones
        xin = C.resize2x(x.astype(np.float32)).astype(np.float64)
        assert np.array_equal(xin, C.resize2x(x)), "the fp32 resize must be exact on these operands"
    ho, wo = -(-xin.shape[1] // stride), -(-xin.shape[2] // stride)
    bias, act1, scale, shift, res, act2 = epilogue_operands(name, o["epi"], cv, (n, ho, wo), o.get("res_pad", 8))
    z, total, lsb = C.conv_split(xin, x2, wt, None, stride, o["x2s"], xb, x2b)
    worst = float(total.max()) / lsb
    assert worst < LIMIT, "%s: sum |terms| / lsb = %.3g 2^24: the accumulator is not exact by construction" % (name, worst / LIMIT)
    if o["mode"] == "int":
        assert np.array_equal(z, C.conv2d(xin, x2, wt, None, stride, o["x2s"])), "int mode: the model IS the convolution"
    z = z[..., :cv]
    if bias is not None:
        z = z + bias
    if o.get("tanh"):
        y = C.epilogue(z, C.ACT_NONE)                                    # the pre-activation; the tanh bar is the test's own
    else:
        y = C.epilogue(z, act1, scale, shift, res, act2)
    r = dict(x=x, xb=xb, x2=x2, x2b=x2b, w=wt, bias=bias, act1=act1, scale=scale, shift=shift, res=res, act2=act2, y=y, cv=cv, ho=ho, wo=wo,
             ymax=float(np.abs(y).max()), worst=worst / LIMIT)
    if o.get("pool"):
        r["yp"] = C.avgpool2(y) if o["pool"] == "avg" else C.maxpool2(y)
    if o.get("proj"):
        rng = np.random.default_rng(seed_of(name) ^ 0xB0)
        proj = rng.integers(-2, 3, size=(3, cout)).astype(np.float64)
        if o["mode"] != "int":                                           # sparse rows: the fp32 sums of fine outputs stay exact
            proj *= rng.random((3, cout)) < 0.125
        yj, tj = C.project(y, proj)
        assert float(tj.max()) / (C.common_lsb(y) * 1.0) < LIMIT, name + ": the projected sums are not exact by construction"
        r["proj"], r["yj"] = proj, yj.astype(np.float32)
        assert np.array_equal(r["yj"].astype(np.float64), yj)
    return r


def descriptor(K, o, r):
    n, c1, c2, cout, k, stride = (o[f] for f in ("n", "c1", "c2", "cout", "k", "stride"))
    h, w = (2 * o["h"], 2 * o["w"]) if o.get("up") else (o["h"], o["w"])
    d = K._conv_desc((n, h, w, c1), (k, k, c1 + c2, cout), stride, c2, o["x2s"], r["cv"])
    d.act1, d.act2 = (C.ACT_TANH, C.ACT_NONE) if o.get("tanh") == "on" else (r["act1"], r["act2"])
    d.algo = K._auto(K.ALGO_AUTO)
    d.y_cstride = r["cv"]
    d.res_cstride = 0 if r["res"] is None else r["res"].shape[3]
    d.prologue = K.PROLOGUE_BILINEAR2X if o.get("up") else K.PROLOGUE_NONE
    d.pool = K.POOL_AVG if o.get("pool") == "avg" else K.POOL_MAX
    return d


def run_forward(K, lib, o, monkeypatch, r=None, ranges=None, preset=None):
    """one planned forward call through the C ABI; every output between guards; returns y (numpy) for the callers that compare runs"""
    for name, value in o["env"].items():
        monkeypatch.setenv(name, value)
    r = r or reference(o)
    name = o["name"]
    d = descriptor(K, o, r)
    has_res = int(r["res"] is not None)
    plan = PLAN[int(lib.shdr_conv2d_plan_f32(ctypes.byref(d), has_res))]
    assert plan == o["plan"], "%s: planned %s, expected %s" % (name, plan, o["plan"])
    what = "%s [%s]" % (name, instance(o))
    st = K._stream()
    # operands
    xd, wd = dev(r["x"]), dev(r["w"])
    x2d = None if r["x2"] is None else dev(r["x2"])
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift", "res")}
    if int(lib.shdr_conv2d_filter_is_plain_f32(ctypes.byref(d), has_res)):
        prepared = wd
    else:
        prepared = torch.empty(int(lib.shdr_conv2d_prepared_filter_elems_f32(ctypes.byref(d), has_res)), device="cuda")
        assert lib.shdr_conv2d_prepare_filter_f32(ctypes.byref(d), has_res, P(wd), P(prepared), st) == 0, lib.shdr_last_error()
    ws = torch.empty(max(int(lib.shdr_conv2d_workspace_bytes_f32(ctypes.byref(d), has_res)), 16), device="cuda", dtype=torch.uint8)
    # range slots of the sources: a declared bound, the measured maximum, or none (measured below the ABI); fine operands need their bound
    ranges = ranges or ("declared" if o["mode"] in ("fx", "fxw") else ("declared", "measured", "none")[seed_of(name) % 3])
    xr1 = xr2 = None
    if ranges == "declared":
        xr1, xr2 = slot_of(r["xb"]), (None if x2d is None else slot_of(r["x2b"]))
    elif ranges == "measured":
        xr1 = slot_of(0.0)
        assert lib.shdr_absmax_f32(P(xd), xd.numel(), P(xr1), st) == 0
        if x2d is not None:
            xr2 = slot_of(0.0)
            assert lib.shdr_absmax_f32(P(x2d), x2d.numel(), P(xr2), st) == 0
    # outputs
    n, ho, wo, cv = o["n"], r["ho"], r["wo"], r["cv"]
    want_y = o.get("pool") != "only" and not (o.get("proj") and not o.get("proj_keeps_y"))
    ybuf = y = None
    if want_y:
        ybuf, y, ynum = guarded_f32((n, ho, wo, cv))
    pbuf = yp = None
    if o.get("pool"):
        pbuf, yp, pnum = guarded_f32((n, ho // 2, wo // 2, cv))
    slot = Slot((seed_of(name) % 4 == 0) * 1.0e6 if preset is None else preset)
    if o.get("proj"):
        pd = dev(r["proj"])
        jbuf, yj, jnum = guarded_f32((n, ho, wo, 3))
        assert int(lib.shdr_conv2d_projected_ok_f32(ctypes.byref(d))) == 1, what
        rc = lib.shdr_conv2d_fwd_prepared_projected_f32(ctypes.byref(d), P(xd), P(x2d), P(prepared), P(opt["bias"]), P(opt["scale"]), P(opt["shift"]),
                                                        P(pd), P(yj), P(y), P(yp), P(ws), P(xr1), P(xr2), P(slot.view), st)
    else:
        rc = lib.shdr_conv2d_fwd_prepared_ranged_f32(ctypes.byref(d), P(xd), P(x2d), P(prepared), P(opt["bias"]), P(opt["scale"]), P(opt["shift"]),
                                                     P(opt["res"]), P(y), P(yp), P(ws), P(xr1), P(xr2), P(slot.view), st)
    assert rc == 0, (what, rc, lib.shdr_last_error())
    where = "pixels" if "1x1_kernel" in instance(o) else "tiles"
    got = None
    if y is not None:
        guards_intact(ybuf, ynum, what + " y")
        got = y.cpu().numpy()
        if o.get("tanh") != "on":
            same(got, r["y"], what + " y", where)
    if yp is not None:
        guards_intact(pbuf, pnum, what + " pooled output")
        same(yp.cpu().numpy(), r["yp"], what + " pooled output (%s)" % o["pool"])
    if o.get("proj"):
        guards_intact(jbuf, jnum, what + " projected output")
        same(yj.cpu().numpy(), r["yj"], what + " projected output")
    if o.get("tanh") != "on":
        slot.check(r["ymax"], what)                                        # (a pooled output carries max |y|, not max |yp|)
    return got, slot


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_x3_kernel<false, 3, 3>: chunks, sources, cout slices, edges, look-ahead, epilogues
# ---------------------------------------------------------------------------------------------------------------------------------
MB = {"SHDR_X3_MIN_BLOCKS": "1"}
X3_3X3 = [
    # 1, 2, 3 and 5 chunks x Cout 64 / 128 / 192; N 1 / 3; H, W from {1, 15, 16, 17, 33}; the four operand modes
    case("x3_c32_64_1x1x1_int", "x3", 1, 1, 1, 32, 0, 64, 3, env=MB),
    case("x3_c32_64_1x15x16_fx_relu", "x3", 1, 15, 16, 32, 0, 64, 3, mode="fx", epi="relu", env=MB),
    case("x3_c64_128_3x16x17_fw_lrelu", "x3", 3, 16, 17, 64, 0, 128, 3, mode="fw", epi="lrelu", env=MB),
    case("x3_c96_192_1x17x15_fxw_affine", "x3", 1, 17, 15, 96, 0, 192, 3, mode="fxw", epi="affine", env=MB),
    case("x3_c160_64_1x33x16_fx_res", "x3", 1, 33, 16, 160, 0, 64, 3, mode="fx", epi="res", env=MB),
    case("x3_c160_64_1x16x33_fxw_act2", "x3", 1, 16, 33, 160, 0, 64, 3, mode="fxw", epi="act2", env=MB),
    case("x3_c64_64_3x1x33_fw_nobias", "x3", 3, 1, 33, 64, 0, 64, 3, mode="fw", epi="nobias", env=MB),
    case("x3_c32_128_1x33x1_int_res", "x3", 1, 33, 1, 32, 0, 128, 3, epi="res", env=MB),
    case("x3_c96_64_1x33x33_fx", "x3", 1, 33, 33, 96, 0, 64, 3, mode="fx", env=MB),
    # two sources: the chunk loop crosses from x1 to x2 (after 1, 2 and 3 chunks); the second source's scale lives in the filter planes
    case("x3_two_32_32_scaled_64_1x17x33_int", "x3", 1, 17, 33, 32, 32, 64, 3, x2s=S8, env=MB),
    case("x3_two_64_32_half_128_3x15x15_fw_relu", "x3", 3, 15, 15, 64, 32, 128, 3, mode="fw", epi="relu", x2s=0.5, env=MB),
    case("x3_two_96_64_scaled_64_1x16x17_fw_affine", "x3", 1, 16, 17, 96, 64, 64, 3, mode="fw", epi="affine", x2s=S8, env=MB),
    case("x3_two_32_32_half_64_1x33x16_fx", "x3", 1, 33, 16, 32, 32, 64, 3, mode="fx", x2s=0.5, env=MB),
    # Cout 32: one 64-cout slice, half of it zero columns that are neither biased nor stored
    case("x3_c64_32_1x17x15_fx_affine", "x3", 1, 17, 15, 64, 0, 32, 3, mode="fx", epi="affine", env=MB),
    case("x3_two_32_32_scaled_32_1x15x16_int_res", "x3", 1, 15, 16, 32, 32, 32, 3, epi="res", x2s=S8, env=MB),
    # the issue orders of the global loads: LOOK 1, and LOOK 2 (the default above) at two more shapes.  The "legacy" cases here and in
    # X3_UP ran the load order of the first rounds until it was removed and run the default order now; they keep
    # their names, which seed their operands
    case("x3_look1_c96_64_1x17x33_fxw", "x3", 1, 17, 33, 96, 0, 64, 3, mode="fxw", env=dict(MB, SHDR_X3_LOOK="1")),
    case("x3_look1_two_32_64_scaled_1x33x15_fw", "x3", 1, 33, 15, 32, 64, 64, 3, mode="fw", x2s=S8, env=dict(MB, SHDR_X3_LOOK="1")),
    case("x3_legacy_c96_128_1x15x17_fxw_res", "x3", 1, 15, 17, 96, 0, 128, 3, mode="fxw", epi="res", env=MB),
    case("x3_legacy_c32_64_3x1x1_fx", "x3", 3, 1, 1, 32, 0, 64, 3, mode="fx", env=MB),
]


@pytest.mark.parametrize("o", X3_3X3)
def test_x3_3x3(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


def test_x3_declines_cout32_under_its_switch_and_another_kernel_answers(K, lib, monkeypatch):
    o = case("x3_cout32_declined", "mfma", 1, 17, 15, 64, 0, 32, 3, epi="relu", env=dict(MB, SHDR_NO_X3_COUT32="1")).values[0]
    run_forward(K, lib, o, monkeypatch)


# pooled / projected outputs of the 3 x 3 form: even H, W including 2 x 2 and 18 x 22
X3_POOLED = [
    case("x3_maxpool_with_y_c32_64_1x2x2_int", "x3", 1, 2, 2, 32, 0, 64, 3, pool="max", env=MB),
    case("x3_maxpool_with_y_c64_128_1x18x22_fx_relu", "x3", 1, 18, 22, 64, 0, 128, 3, mode="fx", epi="relu", pool="max", env=MB),
    case("x3_maxpool_only_c64_64_3x16x34_fw_lrelu", "x3", 3, 16, 34, 64, 0, 64, 3, mode="fw", epi="lrelu", pool="only", env=MB),
    case("x3_maxpool_only_c32_64_1x18x22_fxw", "x3", 1, 18, 22, 32, 0, 64, 3, mode="fxw", pool="only", env=MB),
    case("x3_avgpool_c64_64_1x18x22_fx_relu", "x3", 1, 18, 22, 64, 0, 64, 3, mode="fx", epi="relu", pool="avg", env=MB),
    case("x3_avgpool_two_32_32_half_64_1x2x34_fw", "x3", 1, 2, 34, 32, 32, 64, 3, mode="fw", x2s=0.5, pool="avg", env=MB),
    case("x3_avgpool_cout32_1x18x16_int_affine", "x3", 1, 18, 16, 64, 0, 32, 3, epi="affine", pool="avg", env=MB),
    case("x3_projected_c64_64_1x17x33_int_relu", "x3", 1, 17, 33, 64, 0, 64, 3, epi="relu", proj=True, env=MB),
    case("x3_projected_c32_64_1x15x16_fx", "x3", 1, 15, 16, 32, 0, 64, 3, mode="fx", proj=True, env=MB),
    case("x3_projected_keeps_y_two_32_32_scaled_1x16x17_fw", "x3", 1, 16, 17, 32, 32, 64, 3, mode="fw", x2s=S8, proj=True, proj_keeps_y=True, env=MB),
    case("x3_projected_maxpool_c64_64_1x18x22_int_relu", "x3", 1, 18, 22, 64, 0, 64, 3, epi="relu", proj=True, pool="max", env=MB),
    case("x3_projected_maxpool_c32_64_3x2x2_fx", "x3", 3, 2, 2, 32, 0, 64, 3, mode="fx", proj=True, pool="max", env=MB),
]


@pytest.mark.parametrize("o", X3_POOLED)
def test_x3_pooled_and_projected(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


# conv_x3_kernel<true, 3, 3>: the bilinear 2x prologue.  (h, w) are the LOW-RES sizes; the operand of the convolution is the fp32
# up-sampled image, exact on integer inputs (multiples of 1 / 16).  fine-x does not survive the resize (the blended values leave the
# (k, j) grid and the precondition fails), so the modes are int and fw.
X3_UP = [
    case("x3_up_c32_64_1x1x3_int", "x3", 1, 1, 3, 32, 0, 64, 3, up=True, env=MB),
    case("x3_up_c64_128_1x8x8_fw_relu", "x3", 1, 8, 8, 64, 0, 128, 3, mode="fw", epi="relu", keep=0.5, up=True, env=MB),
    case("x3_up_c96_64_3x9x11_fw_affine", "x3", 3, 9, 11, 96, 0, 64, 3, mode="fw", epi="affine", keep=0.5, up=True, env=MB),
    case("x3_up_c32_128_1x9x11_int_lrelu", "x3", 1, 9, 11, 32, 0, 128, 3, epi="lrelu", up=True, env=MB),
    case("x3_up_projected_c64_64_1x9x11_int_relu", "x3", 1, 9, 11, 64, 0, 64, 3, epi="relu", up=True, proj=True, env=MB),
    case("x3_up_projected_c32_64_1x8x8_fw", "x3", 1, 8, 8, 32, 0, 64, 3, mode="fw", keep=0.3, up=True, proj=True, env=MB),
    case("x3_up_look1_c64_64_1x9x11_fw", "x3", 1, 9, 11, 64, 0, 64, 3, mode="fw", keep=0.5, up=True, env=dict(MB, SHDR_X3_LOOK="1")),
    case("x3_up_legacy_c64_64_1x8x8_fw", "x3", 1, 8, 8, 64, 0, 64, 3, mode="fw", keep=0.5, up=True, env=MB),
    case("x3_up_cout512_materialised_c32_1x9x11_fw", "x3", 1, 9, 11, 32, 0, 512, 3, mode="fw", up=True, env=MB),
    case("x3_up_cout512_in_kernel_c32_1x9x11_fw", "x3", 1, 9, 11, 32, 0, 512, 3, mode="fw", up=True, env=dict(MB, SHDR_X3_UP_ALWAYS="1")),
]


@pytest.mark.parametrize("o", X3_UP)
def test_x3_bilinear_prologue(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_x3_wide_kernel<UP>: the 128-cout blocks (8 waves, the next chunk's patch loaded and split under the MFMAs, pcnt from the pieces of an
# edge tile that lie inside the image, the low-res patch parked and expanded once per 128 couts).  The two switches take the dispatch
# thresholds (256 blocks, 512 couts: speed only) out of the way; `instance()` restates the rule and test_wide_kernel_names asserts it.
# ---------------------------------------------------------------------------------------------------------------------------------
WB = dict(MB, SHDR_X3_WIDE_MIN_BLOCKS="1", SHDR_X3_WIDE_MIN_COUT="128")
XW_3X3 = [
    # 1, 2, 3 and 5 chunks x Cout 128 / 256 / 384; N 1 / 3; the ten SIZES; the four operand modes; every epilogue
    case("xw_c32_128_1x1x1_int", "x3", 1, 1, 1, 32, 0, 128, 3, env=WB),
    case("xw_c64_128_1x15x16_fx_relu", "x3", 1, 15, 16, 64, 0, 128, 3, mode="fx", epi="relu", env=WB),
    case("xw_c96_256_3x16x17_fw_lrelu", "x3", 3, 16, 17, 96, 0, 256, 3, mode="fw", epi="lrelu", env=WB),
    case("xw_c160_128_1x17x15_fxw_affine", "x3", 1, 17, 15, 160, 0, 128, 3, mode="fxw", epi="affine", env=WB),
    case("xw_c32_384_1x33x16_fx_res", "x3", 1, 33, 16, 32, 0, 384, 3, mode="fx", epi="res", env=WB),
    case("xw_c64_256_1x16x33_fxw_act2", "x3", 1, 16, 33, 64, 0, 256, 3, mode="fxw", epi="act2", env=WB),
    case("xw_c96_128_3x1x33_fw_nobias", "x3", 3, 1, 33, 96, 0, 128, 3, mode="fw", epi="nobias", env=WB),
    case("xw_c160_256_1x33x1_int_res", "x3", 1, 33, 1, 160, 0, 256, 3, epi="res", env=WB),
    case("xw_c64_384_1x15x15_fx", "x3", 1, 15, 15, 64, 0, 384, 3, mode="fx", env=WB),
    case("xw_c96_128_1x17x33_fxw_relu", "x3", 1, 17, 33, 96, 0, 128, 3, mode="fxw", epi="relu", env=WB),
    # two sources: the chunk loop crosses from x1 to x2 after 1 and after 2 chunks, the second source at 2^-8 and at 0.5
    case("xw_two_32_32_scaled_128_1x17x33_int", "x3", 1, 17, 33, 32, 32, 128, 3, x2s=S8, env=WB),
    case("xw_two_64_32_half_256_3x15x15_fw_relu", "x3", 3, 15, 15, 64, 32, 256, 3, mode="fw", epi="relu", x2s=0.5, env=WB),
    case("xw_two_32_64_scaled_128_1x16x17_fw_affine", "x3", 1, 16, 17, 32, 64, 128, 3, mode="fw", epi="affine", x2s=S8, env=WB),
    case("xw_two_64_64_half_128_1x33x16_fx_res", "x3", 1, 33, 16, 64, 64, 128, 3, mode="fx", epi="res", x2s=0.5, env=WB),
]
XW_POOLED = [
    case("xw_maxpool_with_y_c32_128_1x2x2_int", "x3", 1, 2, 2, 32, 0, 128, 3, pool="max", env=WB),
    case("xw_maxpool_with_y_c64_256_1x18x22_fx_relu", "x3", 1, 18, 22, 64, 0, 256, 3, mode="fx", epi="relu", pool="max", env=WB),
    case("xw_maxpool_only_c64_128_3x16x34_fw_lrelu", "x3", 3, 16, 34, 64, 0, 128, 3, mode="fw", epi="lrelu", pool="only", env=WB),
    case("xw_maxpool_only_c32_128_1x18x22_fxw", "x3", 1, 18, 22, 32, 0, 128, 3, mode="fxw", pool="only", env=WB),
    case("xw_avgpool_c96_128_1x18x22_fx_relu", "x3", 1, 18, 22, 96, 0, 128, 3, mode="fx", epi="relu", pool="avg", env=WB),
    case("xw_avgpool_two_32_32_half_128_1x2x34_fw", "x3", 1, 2, 34, 32, 32, 128, 3, mode="fw", x2s=0.5, pool="avg", env=WB),
]
# conv_x3_wide_kernel<true>: (h, w) the LOW-RES sizes 1 x 3, 8 x 8 and 9 x 11; modes int and fw (see X3_UP)
XW_UP = [
    case("xw_up_c32_128_1x1x3_int", "x3", 1, 1, 3, 32, 0, 128, 3, up=True, env=WB),
    case("xw_up_c64_256_1x8x8_fw_relu", "x3", 1, 8, 8, 64, 0, 256, 3, mode="fw", epi="relu", keep=0.5, up=True, env=WB),
    case("xw_up_c96_128_3x9x11_fw_affine", "x3", 3, 9, 11, 96, 0, 128, 3, mode="fw", epi="affine", keep=0.5, up=True, env=WB),
    case("xw_up_c32_256_1x9x11_int_lrelu", "x3", 1, 9, 11, 32, 0, 256, 3, epi="lrelu", up=True, env=WB),
    case("xw_up_c64_128_1x9x11_fw_act2", "x3", 1, 9, 11, 64, 0, 128, 3, mode="fw", epi="act2", keep=0.5, up=True, env=WB),
    case("xw_up_c96_256_1x8x8_int_nobias", "x3", 1, 8, 8, 96, 0, 256, 3, epi="nobias", up=True, env=WB),
    case("xw_up_cout512_in_kernel_c32_1x9x11_fw", "x3", 1, 9, 11, 32, 0, 512, 3, mode="fw", up=True, env=dict(WB, SHDR_X3_UP_ALWAYS="1")),
]


@pytest.mark.parametrize("o", XW_3X3 + XW_POOLED + XW_UP)
def test_x3_wide_blocks(K, lib, o, monkeypatch):
    assert ("conv_x3_wide_kernel<true>" if o.get("up") else "conv_x3_wide_kernel<false>") in instance(o) and "resize2x" not in instance(o)
    run_forward(K, lib, o, monkeypatch)


# 1 x 1 layers: conv_x3_1x1_kernel<4> (Cout % 256 == 0), <2> (Cout % 128 == 0), conv_x3_kernel<false, 1, 1> (Cout 64, or SHDR_X3_1X1_SLICED).
# 2, 3, 5 and 16 chunks (the two-deep prefetch at odd and even counts); pixel counts 1, 127, 128, 129, 323; stride 2 at even and odd sizes.
SL = dict(MB, SHDR_X3_1X1_SLICED="1")
X3_1X1 = [
    case("x1_c64_256_1x1x1_fx", "x3", 1, 1, 1, 64, 0, 256, 1, mode="fx", env=MB),
    case("x1_c96_256_1x1x127_fxw_relu", "x3", 1, 1, 127, 96, 0, 256, 1, mode="fxw", epi="relu", env=MB),
    case("x1_c160_128_1x8x16_fw_lrelu", "x3", 1, 8, 16, 160, 0, 128, 1, mode="fw", epi="lrelu", env=MB),
    case("x1_c512_256_1x3x43_fx_affine", "x3", 1, 3, 43, 512, 0, 256, 1, mode="fx", epi="affine", env=MB),
    case("x1_c64_128_1x17x19_fxw_res", "x3", 1, 17, 19, 64, 0, 128, 1, mode="fxw", epi="res", env=MB),
    case("x1_c96_64_1x17x19_fx_res", "x3", 1, 17, 19, 96, 0, 64, 1, mode="fx", epi="res", env=MB),
    case("x1_c160_64_3x1x43_fw", "x3", 3, 1, 43, 160, 0, 64, 1, mode="fw", env=MB),
    case("x1_sliced_c96_256_1x17x19_fxw_res", "x3", 1, 17, 19, 96, 0, 256, 1, mode="fxw", epi="res", env=SL),
    case("x1_sliced_c64_128_1x1x127_fx", "x3", 1, 1, 127, 64, 0, 128, 1, mode="fx", env=SL),
    case("x1_two_32_32_scaled_256_1x3x43_int_relu", "x3", 1, 3, 43, 32, 32, 256, 1, epi="relu", x2s=S8, env=MB),
    case("x1_two_64_96_half_128_1x17x19_fw_res", "x3", 1, 17, 19, 64, 96, 128, 1, mode="fw", epi="res", x2s=0.5, env=MB),
    case("x1_two_32_32_half_64_1x1x127_fw", "x3", 1, 1, 127, 32, 32, 64, 1, mode="fw", x2s=0.5, env=MB),
    case("x1_stride2_c64_256_1x16x16_fx", "x3", 1, 16, 16, 64, 0, 256, 1, stride=2, mode="fx", env=MB),
    case("x1_stride2_c96_128_3x17x15_fxw_affine", "x3", 3, 17, 15, 96, 0, 128, 1, stride=2, mode="fxw", epi="affine", env=MB),
    case("x1_stride2_c64_64_1x33x17_fw", "x3", 1, 33, 17, 64, 0, 64, 1, stride=2, mode="fw", env=MB),
]


@pytest.mark.parametrize("o", X3_1X1)
def test_x3_1x1(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


def test_x3_declines_1x1_with_k32_and_another_kernel_answers(K, lib, monkeypatch):
    o = case("x1_k32_declined", "mfma", 1, 17, 19, 32, 0, 64, 1, epi="relu", env=MB).values[0]
    run_forward(K, lib, o, monkeypatch)


# the 7 x 7 / 2 stem: the MP kernel (four phases of 4 x 4, 4 x 3, 3 x 4 and 3 x 3 taps in one launch).  K = 4704: int mode.  The
# "stem_phases" cases ran the four-launch form until it was removed and run the MP kernel now; they keep their names, which seed their operands.
X3_STEM = [
    case("stem_mp_96_64_1x17x16_relu", "x3", 1, 17, 16, 96, 0, 64, 7, stride=2, epi="relu", env=MB),
    case("stem_mp_96_128_1x32x32_affine", "x3", 1, 32, 32, 96, 0, 128, 7, stride=2, epi="affine", env=MB),
    case("stem_mp_96_64_3x33x35", "x3", 3, 33, 35, 96, 0, 64, 7, stride=2, env=MB),
    case("stem_phases_96_64_1x17x16_affine", "x3", 1, 17, 16, 96, 0, 64, 7, stride=2, epi="affine", env=MB),
    case("stem_phases_96_128_1x33x35_relu", "x3", 1, 33, 35, 96, 0, 128, 7, stride=2, epi="relu", env=MB),
    case("stem_phases_32_64_1x32x32_lrelu", "x3", 1, 32, 32, 32, 0, 64, 7, stride=2, epi="lrelu", env=MB),
]


@pytest.mark.parametrize("o", X3_STEM)
def test_x3_stem(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_x3n_kernel<KK, CT, NT, TWO, TANH>
# ---------------------------------------------------------------------------------------------------------------------------------
X3N = []
_MODES, _EPIS = ("int", "fx", "fw", "fxw"), ("plain", "relu", "lrelu", "affine", "res", "nobias")
for _k in (3, 5, 7):
    for _c1 in (4, 8, 12, 16, 32):
        for _cout in (16, 32):
            if _k == 7 and _c1 == 32:
                continue                                                  # filter + patch over the LDS budget: declined (tested below)
            _i = len(X3N)
            _h, _w = SIZES[_i % len(SIZES)]
            X3N.append(case("x3n_k%d_%d_%d_%dx%dx%d_%s_%s" % (_k, _c1, _cout, 1 + _i % 2, _h, _w, _MODES[_i % 4], _EPIS[_i % 6]), "x3n",
                            1 + _i % 2, _h, _w, _c1, 0, _cout, _k, mode=_MODES[_i % 4], epi=_EPIS[_i % 6], res_pad=4 * (_i % 3), env=MB))
X3N += [
    # two sources 16 + 16 (TWO): the second source's scale folded into the filter rows ch >= C1
    case("x3n_two_k3_16_2x17x33_int_scaled", "x3n", 2, 17, 33, 16, 16, 16, 3, x2s=S8, env=MB),
    case("x3n_two_k3_32_1x15x16_fw_half_relu", "x3n", 1, 15, 16, 16, 16, 32, 3, mode="fw", epi="relu", x2s=0.5, env=MB),
    case("x3n_two_k5_16_1x16x17_fw_scaled_res", "x3n", 1, 16, 17, 16, 16, 16, 5, mode="fw", epi="res", x2s=S8, env=MB),
    case("x3n_two_k5_32_1x33x16_fx_half_affine", "x3n", 1, 33, 16, 16, 16, 32, 5, mode="fx", epi="affine", x2s=0.5, env=MB),
    case("x3n_two_k3_16_1x1x1_fx_scaled", "x3n", 1, 1, 1, 16, 16, 16, 3, mode="fx", x2s=S8, env=MB),
    # the 4 -> 64 image layer <3, 8, 4>
    case("x3n_image64_4_1x17x33_fxw_relu", "x3n", 1, 17, 33, 4, 0, 64, 3, mode="fxw", epi="relu", env=MB),
    case("x3n_image64_8_2x15x15_fx_res", "x3n", 2, 15, 15, 8, 0, 64, 3, mode="fx", epi="res", env=MB),
    # narrow heads: 3 of 16 couts with a residual of 3 channels (the 12-byte path), 5 of 16 (the scalar path)
    case("x3n_head_3_of_16_k3_16_1x17x15_fx_res", "x3n", 1, 17, 15, 16, 0, 16, 3, mode="fx", epi="res", cv=3, res_pad=0, env=MB),
    case("x3n_head_3_of_16_k7_8_1x16x33_fxw_res", "x3n", 1, 16, 33, 8, 0, 16, 7, mode="fxw", epi="res", cv=3, res_pad=0, env=MB),
    case("x3n_head_3_of_16_k3_32_1x33x1_fw", "x3n", 1, 33, 1, 32, 0, 16, 3, mode="fw", cv=3, env=MB),
    case("x3n_head_5_of_16_k5_16_2x15x16_fx_affine", "x3n", 2, 15, 16, 16, 0, 16, 5, mode="fx", epi="affine", cv=5, env=MB),
    case("x3n_head_5_of_16_k3_12_1x17x33_fxw_res", "x3n", 1, 17, 33, 12, 0, 16, 3, mode="fxw", epi="res", cv=5, res_pad=3, env=MB),
    # pooled outputs
    case("x3n_maxpool_k3_16_16_1x18x22_fx_relu", "x3n", 1, 18, 22, 16, 0, 16, 3, mode="fx", epi="relu", pool="max", env=MB),
    case("x3n_maxpool_k5_32_32_1x2x2_fw", "x3n", 1, 2, 2, 32, 0, 32, 5, mode="fw", pool="max", env=MB),
    case("x3n_avgpool_k3_two_16_16_32_1x18x22_fw_lrelu", "x3n", 1, 18, 22, 16, 16, 32, 3, mode="fw", epi="lrelu", x2s=0.5, pool="avg", env=MB),
    case("x3n_avgpool_k7_4_16_2x16x34_fxw", "x3n", 2, 16, 34, 4, 0, 16, 7, mode="fxw", pool="avg", env=MB),
    case("x3n_avgpool_image64_4_1x34x18_fx_res", "x3n", 1, 34, 18, 4, 0, 64, 3, mode="fx", epi="res", pool="avg", env=MB),
]


@pytest.mark.parametrize("o", X3N)
def test_x3n(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


@pytest.mark.parametrize("c1,c2,cout", [(32, 0, 32), (32, 0, 16), (16, 16, 16)])
def test_x3n_declines_7x7_over_the_lds_budget_and_another_kernel_answers(K, lib, monkeypatch, c1, c2, cout):
    o = case("x3n_k7_%d_%d_%d_declined" % (c1, c2, cout), "mfma", 1, 17, 15, c1, c2, cout, 7, epi="relu", x2s=0.5 if c2 else 1.0, env=MB).values[0]
    run_forward(K, lib, o, monkeypatch)


def test_x3n_declines_the_image_layer_under_its_switch(K, lib, monkeypatch):
    o = case("x3n_image64_declined", "mfma", 1, 17, 15, 4, 0, 64, 3, epi="relu", env=dict(MB, SHDR_NO_X3N_IMAGE64="1")).values[0]
    run_forward(K, lib, o, monkeypatch)


# tanh heads (the 16-cout single-source instantiations, tanh_fast of shdr_internal.h).  The pre-activation -- the same case with ACT_NONE --
# is exact; the tanh output is held to the claim written next to tanh_fast: |got - tanh(pre)| <= one fp32 ulp + 1e-6 |tanh(pre)|.
TANH = [
    case("x3n_tanh_k3_16_3_of_16_1x33x33_fx", "x3n", 1, 33, 33, 16, 0, 16, 3, mode="fx", cv=3, tanh="pre", env=MB),
    case("x3n_tanh_k3_8_16_1x17x33_fx", "x3n", 1, 17, 33, 8, 0, 16, 3, mode="fx", tanh="pre", env=MB),
    case("x3n_tanh_k5_32_16_1x16x17_fxw", "x3n", 1, 16, 17, 32, 0, 16, 5, mode="fxw", tanh="pre", env=MB),
    case("x3n_tanh_k7_16_5_of_16_1x15x16_fx", "x3n", 1, 15, 16, 16, 0, 16, 7, mode="fx", cv=5, tanh="pre", env=MB),
]


@pytest.mark.parametrize("o", TANH)
def test_x3n_tanh_heads(K, lib, o, monkeypatch):
    r = reference(o)
    cv = r["cv"]
    # small dyadic biases spread the pre-activations over (0, 0.1), [0.1, 4] and exact zeros (column 1: no weights, no bias)
    bias = np.array([0.0, 0.0, 2.0 ** -5, 0.5, -1.0, 2.0, -3.0, 2.0 ** -7, 1.5, -0.25, 3.5, 0.0, 0.75, -2.0 ** -4, 1.0, -0.5])[:cv]
    r["w"][..., 1] = 0.0
    z = C.conv_split(r["x"], None, r["w"], None, 1, 1.0, r["xb"])[0][..., :cv] + bias
    r["bias"], r["y"] = bias, C.epilogue(z, C.ACT_NONE)
    r["ymax"] = float(np.abs(r["y"]).max())
    pre = r["y"].astype(np.float64)
    a = np.abs(pre)
    assert (pre[..., 1] == 0).all() and ((a > 0) & (a < 0.1)).sum() >= 50 and ((a >= 0.1) & (a <= 4)).sum() >= 200
    run_forward(K, lib, dict(o, tanh="pre"), monkeypatch, r=r)           # ACT_NONE: the pre-activation, bit for bit
    got, slot = run_forward(K, lib, dict(o, tanh="on"), monkeypatch, r=r)
    want = np.tanh(pre)
    bar = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-6 * np.abs(want)
    frac = np.abs(got.astype(np.float64) - want) / bar
    i = np.unravel_index(int(np.argmax(frac)), frac.shape)
    print("%s: worst |got - tanh(pre)| = %.3f of the bar, at pre = %r (got %r, tanh %r); worst below 0.1: %.3f"
          % (o["name"], frac.max(), float(pre[i]), float(got[i]), float(want[i]), float(frac[a < 0.1].max())))
    assert (got[..., 1] == 0).all(), "tanh(0) must be 0"
    # the range slot of the tanh head: the largest stored value, bit for bit, and max |tanh(pre)| at the same bar
    top = float(np.abs(want).max())
    slot.check(float(np.abs(got).max()), o["name"] + " (tanh output)")
    assert abs(float(np.abs(got).max()) - top) <= float(np.spacing(np.float32(top))) + 1e-6 * top, "range slot of the tanh head misses max |tanh(pre)|"
    assert float(frac.max()) <= 1.0, "tanh_fast misses its documented bar at pre = %r: got %r, tanh %r (%.3f of the bar)" % (
        float(pre[i]), float(got[i]), float(want[i]), float(frac.max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the persistent tile loop of conv_x3n_kernel: 1 x 528 x 512 = 1056 tiles, more than the 256 x 4 persistent blocks of the largest grid and
# not a multiple of any grid.  A block's second tile runs the prefetch under the MFMAs and patch_wait(stores_since) in its three forms.
# ---------------------------------------------------------------------------------------------------------------------------------
BIG = dict(n=1, h=528, w=512)
_BIG_REF = {}


def big_reference(o):
    """the float64 model of the big 16 -> 16 layer is computed once and shared by its four forms (the filter differs only in the zeroed
    columns of the 3-of-16 head, which change neither S nor the kept columns)"""
    key = (o["c1"], o["c2"], o["cout"])
    if key not in _BIG_REF:
        base = dict(o, name="x3n_big_%d_%d_%d" % key, epi="plain", cv=None, pool=None)
        _BIG_REF[key] = reference(base)
    b = _BIG_REF[key]
    cv = o.get("cv") or o["cout"]
    bias, act1, scale, shift, res, act2 = epilogue_operands(o["name"], o["epi"], cv, (1, 528, 512), 0)
    w = b["w"].copy()
    w[..., cv:] = 0.0
    z = b["y"].astype(np.float64)[..., :cv]                               # the base ran the plain epilogue: its bias goes, this form's comes
    z = z - b["bias"][:cv] + (0.0 if bias is None else bias)
    y = C.epilogue(z, act1, scale, shift, res, act2)
    r = dict(b, w=w, bias=bias, act1=act1, scale=scale, shift=shift, res=res, act2=act2, y=y, cv=cv, ymax=float(np.abs(y).max()))
    if o.get("pool"):
        r["yp"] = C.maxpool2(y)
    return r


X3N_BIG = [
    case("x3n_big_plain_stores_full", "x3n", 1, 528, 512, 16, 0, 16, 3, epi="relu"),
    case("x3n_big_pooled_stores_three_halves", "x3n", 1, 528, 512, 16, 0, 16, 3, epi="relu", pool="max"),
    case("x3n_big_residual_drains", "x3n", 1, 528, 512, 16, 0, 16, 3, epi="res"),
    case("x3n_big_head_3_of_16_drains", "x3n", 1, 528, 512, 16, 0, 16, 3, epi="plain", cv=3),
]


@pytest.mark.parametrize("o", X3N_BIG)
def test_x3n_persistent_loop(K, lib, o, monkeypatch):
    assert (528 // 16) * (512 // 16) == 1056
    run_forward(K, lib, o, monkeypatch, r=big_reference(o), ranges="declared")


X3N_BIG_OTHER = [case("x3n_big_two_16_16_scaled", "x3n", 1, 528, 512, 16, 16, 16, 3, epi="relu", x2s=S8),
                 case("x3n_big_image64_4", "x3n", 1, 528, 512, 4, 0, 64, 3, epi="relu")]


@pytest.mark.parametrize("o", X3N_BIG_OTHER)
def test_x3n_persistent_loop_two_sources_and_image_layer(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch, ranges="declared")


# ---------------------------------------------------------------------------------------------------------------------------------
# the input gradient (shdr_conv2d_dgrad_ranged_f32): filter transform (flip, slice, the source's scale), then the same kernels on dz
# ---------------------------------------------------------------------------------------------------------------------------------
def dcase(name, kernel, n, h, w, c1, c2, cout, k, which, mode="int", x2s=1.0, ranges=None, env=MB):
    return pytest.param(dict(name=name, kernel=kernel, n=n, h=h, w=w, c1=c1, c2=c2, cout=cout, k=k, which=which, mode=mode, x2s=x2s,
                             ranges=ranges, env=env), id=name)


DGRAD = [
    # conv_x3_kernel<false, 3, 3>: Cx 64 / 128 from Cout 32 m
    dcase("dgrad_x3_cx64_from_32_1x17x15_int", "x3", 1, 17, 15, 64, 0, 32, 3, 0, ranges="measured"),
    dcase("dgrad_x3_cx128_from_64_1x15x16_fx", "x3", 1, 15, 16, 128, 0, 64, 3, 0, mode="fx"),
    dcase("dgrad_x3_cx64_from_96_3x16x17_fw", "x3", 3, 16, 17, 64, 0, 96, 3, 0, mode="fw", ranges="measured"),
    dcase("dgrad_x3_cx128_from_160_1x33x16_fxw", "x3", 1, 33, 16, 128, 0, 160, 3, 0, mode="fxw"),
    dcase("dgrad_x3_two_64_64_which1_scaled_from_64_1x17x33_int", "x3", 1, 17, 33, 64, 64, 64, 3, 1, x2s=S8, ranges="none"),
    dcase("dgrad_x3_two_64_128_which1_scaled_from_32_1x15x15_fx", "x3", 1, 15, 15, 64, 128, 32, 3, 1, mode="fx", x2s=S8),
    dcase("dgrad_x3_two_128_64_which0_from_64_1x16x33_fw", "x3", 1, 16, 33, 128, 64, 64, 3, 0, mode="fw", x2s=S8, ranges="none"),
    # conv_x3n_kernel: the 16 + 16 -> 16 layers, both sources, k 3 / 5 / 7
    dcase("dgrad_x3n_k3_two_which0_scaled_1x17x33_int", "x3n", 1, 17, 33, 16, 16, 16, 3, 0, x2s=S8, ranges="measured"),
    dcase("dgrad_x3n_k3_two_which1_scaled_1x17x33_fx", "x3n", 1, 17, 33, 16, 16, 16, 3, 1, mode="fx", x2s=S8),
    dcase("dgrad_x3n_k3_two_which1_half_2x15x16_fw", "x3n", 2, 15, 16, 16, 16, 16, 3, 1, mode="fw", x2s=0.5, ranges="none"),
    dcase("dgrad_x3n_k5_two_which0_half_1x16x17_fx", "x3n", 1, 16, 17, 16, 16, 16, 5, 0, mode="fx", x2s=0.5),
    dcase("dgrad_x3n_k5_two_which1_scaled_1x33x16_fxw", "x3n", 1, 33, 16, 16, 16, 16, 5, 1, mode="fxw", x2s=S8),
    dcase("dgrad_x3n_k7_two_which0_scaled_1x15x15_fw", "x3n", 1, 15, 15, 16, 16, 16, 7, 0, mode="fw", x2s=S8, ranges="measured"),
    dcase("dgrad_x3n_k7_two_which1_half_1x1x33_fx", "x3n", 1, 1, 33, 16, 16, 16, 7, 1, mode="fx", x2s=0.5),
    dcase("dgrad_x3n_k7_two_which1_scaled_1x16x33_int", "x3n", 1, 16, 33, 16, 16, 16, 7, 1, x2s=S8, ranges="none"),
    dcase("dgrad_x3n_k3_32_from_32_1x17x15_fxw", "x3n", 1, 17, 15, 32, 0, 32, 3, 0, mode="fxw"),
    dcase("dgrad_x3n_k5_16_from_4_of_16_1x15x16_fx", "x3n", 1, 15, 16, 16, 0, 4, 5, 0, mode="fx"),
]


# the transposed layer dz -> dx of a Cx = 128 source runs x3_forward with 128 couts: under the two switches the 128-cout blocks take it
# (test_wide_kernel_names asserts the kernel by name)
DGRAD_WIDE = [dcase("dgrad_xw_cx128_from_64_1x17x15_fx", "x3", 1, 17, 15, 128, 0, 64, 3, 0, mode="fx", env=WB),
              dcase("dgrad_xw_two_64_128_which1_scaled_from_96_3x15x16_fw", "x3", 3, 15, 16, 64, 128, 96, 3, 1, mode="fw", x2s=S8, ranges="none", env=WB)]


def dgrad_reference(o):
    n, h, w, c1, c2, cout, k, which, x2s = (o[f] for f in ("n", "h", "w", "c1", "c2", "cout", "k", "which", "x2s"))
    rng = np.random.default_rng(seed_of(o["name"]))
    dz, zb = fine_x(rng, (n, h, w, cout))[:2] if o["mode"] in ("fx", "fxw") else int_x(rng, (n, h, w, cout))
    shape = (k, k, c1 + c2, cout)
    wt = fine_w(rng, shape)[0] if o["mode"] in ("fw", "fxw") else int_w(rng, shape)
    cb, cc, s = (c1, c2, x2s) if which else (0, c1, 1.0)
    if not wt[:, :, cb:cb + cc].any() or np.abs(wt[:, :, cb:cb + cc]).max() != 1.0:
        wt[0, 0, cb, 0] = 1.0                                            # the largest element of the SLICE fixes S of the transposed filter
    # conv_ref.dgrad semantics through filter_transform (dgrad_filter_kernel: ONE fp32 product with the source's scale) + conv_split on dz
    filt = C.filter_transform(wt, cb, cc, s)
    assert np.array_equal(filt.astype(np.float32).astype(np.float64), filt)
    dx, total, lsb = C.conv_split(dz, None, filt, None, 1, 1.0, zb)
    worst = float(total.max()) / lsb
    assert worst < LIMIT, "%s: sum |terms| / lsb = %.3g 2^24" % (o["name"], worst / LIMIT)
    if o["mode"] == "int":
        assert np.array_equal(dx, C.dgrad(dz, wt, (n, h, w, cc), cb, cc, s, 1)), "int mode: the model IS the input gradient"
    return dz, zb, wt, dx.astype(np.float32), cc


@pytest.mark.parametrize("o", DGRAD + DGRAD_WIDE)
def test_input_gradient(K, lib, o, monkeypatch):
    for name, value in o["env"].items():
        monkeypatch.setenv(name, value)
    dz, zb, wt, dx_ref, cc = dgrad_reference(o)
    n, h, w = o["n"], o["h"], o["w"]
    cv = o["cout"]
    cout = 16 if cv < 16 else cv                                          # (a 4-of-16 head: the filter tensor is padded, dz carries 4 channels)
    if cout != cv:
        wt = np.concatenate([wt, np.zeros(wt.shape[:3] + (cout - cv,))], -1)
    d = K._conv_desc((n, h, w, o["c1"]), (o["k"], o["k"], o["c1"] + o["c2"], cout), 1, o["c2"], o["x2s"], cv)
    d.algo = K._auto(K.ALGO_AUTO)
    # the kernel the transposed layer takes, by dgrad_geom: x3n where the narrow predicate takes (dz channels -> Cx), else x3 where the
    # fused-Winograd shape rule and the wide predicate do; both write the range slot of dx from their epilogue
    t = K._conv_desc((n, h, w, cv), (o["k"], o["k"], cv, cc), 1, 0, 1.0, cc)
    t.algo, t.y_cstride = d.algo, 0
    assert PLAN[int(lib.shdr_conv2d_plan_f32(ctypes.byref(t), 0))] == o["kernel"], o["name"]
    assert int(lib.shdr_conv2d_dgrad_tracks_range_f32(ctypes.byref(d), o["which"])) == 1
    what = "%s [%s on dz]" % (o["name"], o["kernel"])
    ws = torch.empty(max(int(lib.shdr_conv2d_dgrad_workspace_bytes_f32(ctypes.byref(d), o["which"])), 16), device="cuda", dtype=torch.uint8)
    dzd, wd = dev(dz), dev(wt)
    ranges = o["ranges"] or "declared"
    assert ranges == "declared" or o["mode"] in ("int", "fw"), "a fine dz needs its declared bound"
    zr = None
    if ranges == "declared":
        zr = slot_of(zb)
    elif ranges == "measured":
        zr = slot_of(0.0)
        assert lib.shdr_absmax_f32(P(dzd), dzd.numel(), P(zr), K._stream()) == 0
    buf, dx, numel = guarded_f32((n, h, w, cc))
    slot = Slot((seed_of(o["name"]) % 3 == 0) * 1.0e6)
    rc = lib.shdr_conv2d_dgrad_ranged_f32(ctypes.byref(d), o["which"], P(dzd), P(wd), P(dx), P(ws), P(zr), P(slot.view), K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    guards_intact(buf, numel, what + " dx")
    same(dx.cpu().numpy(), dx_ref, what + " dx")
    slot.check(float(np.abs(dx_ref).max()), what)


def named(name):
    for p in X3_3X3 + X3_POOLED + X3_UP + XW_3X3 + XW_POOLED + XW_UP + X3_1X1 + X3_STEM + X3N + TANH + X3N_BIG + X3N_BIG_OTHER + DGRAD + DGRAD_WIDE:
        if p.id == name:
            return p
    raise KeyError(name)


def kernels_of(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if "conv_x3" in e.name}


def test_wide_kernel_names(K, lib, monkeypatch):
    """the library exports the plan, not the instantiation: the kernels this file's switches launch, by name.  Plain, with the prologue
    and on the input gradient the 128-cout blocks answer; under SHDR_X3_SLICED=1 the 64-cout kernel does."""
    plain, up, dg = named("xw_c64_128_1x15x16_fx_relu").values[0], named("xw_up_c64_256_1x8x8_fw_relu").values[0], named("dgrad_xw_cx128_from_64_1x17x15_fx")
    for o, tag in ((plain, "conv_x3_wide_kernel<false>"), (up, "conv_x3_wide_kernel<true>")):
        r = reference(o)
        names = kernels_of(lambda: run_forward(K, lib, o, monkeypatch, r=r))
        assert any(tag in k for k in names) and not any("conv_x3_kernel" in k for k in names), (o["name"], names)
        sliced = dict(o, env=dict(o["env"], SHDR_X3_SLICED="1"))
        assert "wide" not in instance(sliced)
        names = kernels_of(lambda: run_forward(K, lib, sliced, monkeypatch, r=r))
        own = "conv_x3_kernel<%s" % ("true" if o.get("up") else "false")
        assert any(own in k for k in names) and not any("conv_x3_wide_kernel" in k for k in names), names
        monkeypatch.delenv("SHDR_X3_SLICED")
    names = kernels_of(lambda: test_input_gradient(K, lib, dg.values[0], monkeypatch))
    assert any("conv_x3_wide_kernel<false>" in k for k in names) and not any("conv_x3_kernel" in k for k in names), names
    # without the two switches the same layer stays on the 64-cout kernel (one block of 128 couts, far below 256)
    monkeypatch.delenv("SHDR_X3_WIDE_MIN_BLOCKS")
    monkeypatch.delenv("SHDR_X3_WIDE_MIN_COUT")
    o = dict(plain, env=MB)
    assert "wide" not in instance(o)
    names = kernels_of(lambda: run_forward(K, lib, o, monkeypatch, r=reference(plain)))
    assert names and not any("conv_x3_wide_kernel" in k for k in names), names


# ---------------------------------------------------------------------------------------------------------------------------------
# range slots: a declared bound, the producer's slot and the measured range give the same y; the Python wrapper
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", [named(n) for n in ("x3_c32_64_1x1x1_int", "x3_two_32_32_scaled_64_1x17x33_int", "x1_two_32_32_scaled_256_1x3x43_int_relu",
                                                  "x3n_two_k3_16_2x17x33_int_scaled", "stem_mp_96_64_1x17x16_relu")])
def test_declared_measured_and_absent_ranges_give_the_same_output(K, lib, o, monkeypatch):
    assert o["mode"] == "int"
    r = reference(o)
    for ranges in ("declared", "measured", "none"):
        for preset in (0.0, 1.0e6):
            run_forward(K, lib, o, monkeypatch, r=r, ranges=ranges, preset=preset)


# Unusual slot contents in front of every forward reader of a range slot (all of them take T from shdr::range_exponent, csrc/split.h; the
# split pass of the weight gradient has test_split_planes_slots, the one-launch low-res form tests/test_gpu_up2_narrow.py): the smallest
# int-mode case of conv_x3_kernel, its bilinear-prologue form, conv_x3_1x1_kernel, conv_x3_wide_kernel and conv_x3n_kernel under an
# empty slot, infinity, a NaN pattern, a word with the sign bit set (all four: T = 0, the input is split as it stands), a bound that is
# no power of two and a large one (T = 9 and -5).  A second source holds integers / x2_scale, so its slot holds bound / x2_scale as the
# harness's own declared bounds do (the same word in both slots would push that source out of the fp16 range and fail the
# precondition); the slots without a bound go into both as they are.  The two-source cases also take the mixed pairs, in which the
# larger BIT PATTERN wins and the launch runs unscaled.  The precondition of `reference` holds for every pair below.
NAN_SLOT = np.uint32(0x7FC5A5A5).view(np.float32)
SLOT_CONTENTS = [("zero", 0.0), ("inf", np.float32(np.inf)), ("nan_bits", NAN_SLOT), ("sign_bit", -3.0), ("three", 3.0), ("large", 6.0e4)]
SLOT_READERS = ("x3_c32_64_1x1x1_int", "x3_up_c32_64_1x1x3_int", "x1_two_32_32_scaled_256_1x3x43_int_relu", "xw_c32_128_1x1x1_int",
                "x3n_two_k3_16_2x17x33_int_scaled")


def slot_cases():
    out = []
    for o in (named(n).values[0] for n in SLOT_READERS):
        for tag, b in SLOT_CONTENTS:
            has_bound = bool(np.isfinite(b)) and b > 0
            out.append(pytest.param(o, (b, (b / o["x2s"] if has_bound else b) if o["c2"] else None), id="%s-%s" % (o["name"], tag)))
        if o["c2"]:
            out.append(pytest.param(o, (np.float32(np.inf), 2.0), id=o["name"] + "-inf_and_two"))
            out.append(pytest.param(o, (2.0, NAN_SLOT), id=o["name"] + "-two_and_nan_bits"))
    return out


@pytest.mark.parametrize("o, bounds", slot_cases())
def test_unusual_slot_contents(K, lib, o, bounds, monkeypatch):
    assert o["mode"] == "int"
    run_forward(K, lib, o, monkeypatch, r=reference(o, bounds), ranges="declared")


@pytest.mark.parametrize("o", [named(n) for n in ("x3_c64_128_3x16x17_fw_lrelu", "x1_c96_256_1x1x127_fxw_relu", "x1_c64_128_1x17x19_fxw_res",
                                                  "x3n_two_k5_32_1x33x16_fx_half_affine", "x3n_image64_4_1x17x33_fxw_relu")])
def test_wrapper_writes_out_between_guards_and_hands_the_slot_on(K, lib, o, monkeypatch):
    """shdr._ops.conv2d(out=view): y through the Python wrapper, into a view between guards; the tensor's range record is the slot the
    kernel wrote (the producer's slot that the next layer reads)."""
    for name, value in o["env"].items():
        monkeypatch.setenv(name, value)
    r = reference(o)
    xd = K.set_bound(dev(r["x"]), r["xb"])
    x2d = None if r["x2"] is None else K.set_bound(dev(r["x2"]), r["x2b"])
    buf, y, numel = guarded_f32(r["y"].shape)
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift", "res")}
    wd = dev(r["w"])
    assert K.conv2d_plan(tuple(xd.shape), tuple(wd.shape), c2=o["c2"], stride=o["stride"], x2_scale=o["x2s"], has_residual=r["res"] is not None) == o["plan"]
    out = K.conv2d(xd, wd, opt["bias"], o["stride"], x2d, o["x2s"], r["act1"], opt["scale"], opt["shift"], opt["res"], r["act2"], out=y)
    guards_intact(buf, numel, o["name"] + " y through out=")
    same(out.cpu().numpy(), r["y"], o["name"] + " y through out=")
    slot = K._range_of(out)
    assert slot is not None and bits32(slot.cpu().numpy()) == bits32(r["ymax"]), "the wrapper's range record is not max |y_ref|"


def test_producer_slot_feeds_the_next_layer(K, lib, monkeypatch):
    """two chained layers through the C ABI: the range slot the first layer's epilogue wrote is handed to the second as its x1_range.
    The first layer's integers reach up to 2^7, so the slot (max |y1|, T = 11 - its frexp exponent) differs from any bound of the other
    tests; a declared bound of the next power of two and the measured range give the same second output, bit for bit."""
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    o1 = dict(case("chain_first_c32_64_1x17x15_int_relu", "x3", 1, 17, 15, 32, 0, 64, 3, epi="relu").values[0])
    r1 = reference(o1)
    y1 = r1["y"].astype(np.float64)
    rng = np.random.default_rng(seed_of("chain_second"))
    bound = float(2.0 ** np.ceil(np.log2(r1["ymax"]) + 1e-9))
    # first layer: y1 and its slot
    st = K._stream()
    d1 = descriptor(K, o1, r1)
    assert PLAN[int(lib.shdr_conv2d_plan_f32(ctypes.byref(d1), 0))] == "x3"
    xd, w1d, b1d = dev(r1["x"]), dev(r1["w"]), dev(r1["bias"])
    p1 = torch.empty(int(lib.shdr_conv2d_prepared_filter_elems_f32(ctypes.byref(d1), 0)), device="cuda")
    assert lib.shdr_conv2d_prepare_filter_f32(ctypes.byref(d1), 0, P(w1d), P(p1), st) == 0
    ws = torch.empty(4096, device="cuda", dtype=torch.uint8)
    b1, y1d, n1 = guarded_f32(r1["y"].shape)
    s1 = Slot(0.0)
    assert lib.shdr_conv2d_fwd_prepared_ranged_f32(ctypes.byref(d1), P(xd), None, P(p1), P(b1d), None, None, None, P(y1d), None, P(ws),
                                                   P(slot_of(r1["xb"])), None, P(s1.view), st) == 0, lib.shdr_last_error()
    guards_intact(b1, n1, "chain: y1")
    same(y1d.cpu().numpy(), r1["y"], "chain: y1")
    s1.check(r1["ymax"], "chain: y1")
    # second layer, 64 -> 64 on the wide kernel: its input is the first layer's output AS IT LIES ON THE DEVICE
    w2 = int_w(rng, (3, 3, 64, 64))
    y2_ref = None
    assert C.range_exponent(bound) != C.range_exponent(r1["ymax"])
    for b in (r1["ymax"], bound):                                        # T differs between the two bounds; the integers stay exact under both
        z2, total, lsb = C.conv_split(y1, None, w2, None, 1, 1.0, b)
        assert float(total.max()) / lsb < LIMIT and np.array_equal(z2, C.conv2d(y1, None, w2, None, 1, 1.0))
        assert y2_ref is None or np.array_equal(y2_ref, C.epilogue(z2, C.ACT_NONE))
        y2_ref = C.epilogue(z2, C.ACT_NONE)
    d2 = K._conv_desc((1, 17, 15, 64), (3, 3, 64, 64), 1, 0, 1.0, None)
    d2.algo, d2.y_cstride = K._auto(K.ALGO_AUTO), 64
    assert PLAN[int(lib.shdr_conv2d_plan_f32(ctypes.byref(d2), 0))] == "x3"
    w2d = dev(w2)
    p2 = torch.empty(int(lib.shdr_conv2d_prepared_filter_elems_f32(ctypes.byref(d2), 0)), device="cuda")
    assert lib.shdr_conv2d_prepare_filter_f32(ctypes.byref(d2), 0, P(w2d), P(p2), st) == 0
    measured = slot_of(0.0)
    assert lib.shdr_absmax_f32(P(y1d), y1d.numel(), P(measured), st) == 0
    declared = slot_of(bound)
    for what, xr in (("the producer's slot", s1.view), ("the measured range", measured), ("a declared bound", declared), ("no slot", None)):
        b2, y2d, n2 = guarded_f32(y2_ref.shape)
        s2 = Slot(0.0)
        assert lib.shdr_conv2d_fwd_prepared_ranged_f32(ctypes.byref(d2), P(y1d), None, P(p2), None, None, None, None, P(y2d), None, P(ws),
                                                       P(xr), None, P(s2.view), st) == 0, lib.shdr_last_error()
        guards_intact(b2, n2, "chain: y2 with " + what)
        same(y2d.cpu().numpy(), y2_ref, "chain: y2 with " + what)
        s2.check(float(np.abs(y2_ref).max()), "chain: y2 with " + what)
    s1.check(r1["ymax"], "chain: the producer's slot after the consumer read it")


def test_wrapper_input_gradient(K, lib, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    for o in (named("dgrad_x3_two_64_128_which1_scaled_from_32_1x15x15_fx").values[0], named("dgrad_x3n_k5_two_which1_scaled_1x33x16_fxw").values[0]):
        dz, zb, wt, dx_ref, cc = dgrad_reference(o)
        dzd = K.set_bound(dev(dz), zb)
        dx = K.conv2d_dgrad(dzd, dev(wt), (o["n"], o["h"], o["w"], cc), o["c1"], o["c2"], o["which"], 1, o["x2s"])
        same(dx.cpu().numpy(), dx_ref, o["name"] + " through the wrapper")
        assert bits32(K._range_of(dx).cpu().numpy()) == bits32(np.abs(dx_ref).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: the documented code comes back and the sentinel outputs are untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(K, lib, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    n, h, w, c, cout = 1, 16, 18, 64, 64
    x = torch.zeros((n * h * w * c + 8,), device="cuda")
    filt = torch.zeros((16 + 9 * 128 * 128,), device="cuda")
    vec = torch.zeros((256 + 8,), device="cuda")
    res = torch.zeros((n * h * w * (cout + 8) + 8,), device="cuda")
    sl = slot_of(2.0)
    ybuf, y, _ = guarded_f32((n, h, w, cout))
    pbuf, yp, _ = guarded_f32((n, h // 2, w // 2, cout))
    jbuf, yj, _ = guarded_f32((n, h, w, 3))
    rbuf = Slot(0.0)
    st = K._stream()

    def desc(c1=c, c2=0, co=cout, k=3, hh=h, ww=w, **kw):
        d = K._conv_desc((n, hh, ww, c1), (k, k, c1 + c2, co), 1, c2, 1.0, kw.pop("cv", None))
        d.algo = K._auto(K.ALGO_AUTO)
        d.y_cstride = d.cout_valid
        for f, v in kw.items():
            setattr(d, f, v)
        return d

    def refused(rc, code, what):
        assert rc == code, (what, rc, code, lib.shdr_last_error())
        for b in (ybuf, pbuf, jbuf):
            untouched(b, what)
        rbuf.check(0.0, what)

    x3, x3r, x3p, x3n = (lib.shdr_conv2d_fwd_x3_ranged_f32, lib.shdr_conv2d_fwd_x3_residual_f32, lib.shdr_conv2d_fwd_x3_projected_f32,
                         lib.shdr_conv2d_fwd_x3n_ranged_f32)
    good = desc()
    assert lib.shdr_conv2d_x3_ok_f32(ctypes.byref(good)) == 1
    R = P(rbuf.view)
    # conv_x3: misaligned pointers
    refused(x3(ctypes.byref(good), P(x, 4), None, P(filt), P(vec), None, None, P(y), None, P(sl), None, R, st), E_ALIGN, "x3: x1 misaligned")
    refused(x3(ctypes.byref(good), P(x), None, P(filt, 8), P(vec), None, None, P(y), None, P(sl), None, R, st), E_ALIGN, "x3: filter misaligned")
    refused(x3(ctypes.byref(good), P(x), None, P(filt), P(vec, 4), None, None, P(y), None, P(sl), None, R, st), E_ALIGN, "x3: bias misaligned")
    refused(x3(ctypes.byref(good), P(x), None, P(filt), P(vec), P(vec), P(vec, 12), P(y), None, P(sl), None, R, st), E_ALIGN, "x3: shift misaligned")
    refused(x3(ctypes.byref(good), P(x), None, P(filt), P(vec), None, None, P(y, 4), None, P(sl), None, R, st), E_ALIGN, "x3: y misaligned")
    refused(x3(ctypes.byref(desc(c2=64)), P(x), P(x, 8), P(filt), P(vec), None, None, P(y), None, P(sl), P(sl), R, st), E_ALIGN, "x3: x2 misaligned")
    # x2 iff C2; scale without shift; ranges of both sources or of neither
    refused(x3(ctypes.byref(good), P(x), P(x), P(filt), P(vec), None, None, P(y), None, P(sl), P(sl), R, st), E_NULL, "x3: x2 without C2")
    refused(x3(ctypes.byref(desc(c2=64)), P(x), None, P(filt), P(vec), None, None, P(y), None, P(sl), None, R, st), E_NULL, "x3: C2 without x2")
    refused(x3(ctypes.byref(good), P(x), None, P(filt), P(vec), P(vec), None, P(y), None, P(sl), None, R, st), E_NULL, "x3: scale without shift")
    refused(x3(ctypes.byref(good), P(x), None, P(filt), P(vec), None, P(vec), P(y), None, P(sl), None, R, st), E_NULL, "x3: shift without scale")
    refused(x3(ctypes.byref(desc(c2=64)), P(x), P(x), P(filt), P(vec), None, None, P(y), None, P(sl), None, R, st), E_NULL, "x3: one range of two")
    refused(x3(ctypes.byref(good), P(x), None, P(filt), P(vec), None, None, None, None, P(sl), None, R, st), E_NULL, "x3: no output")
    # odd H with a pooled output
    refused(x3(ctypes.byref(desc(hh=15)), P(x), None, P(filt), P(vec), None, None, P(y), P(yp), P(sl), None, R, st), E_SHAPE, "x3: odd H, pooled")
    refused(x3(ctypes.byref(desc(ww=17)), P(x), None, P(filt), P(vec), None, None, None, P(yp), P(sl), None, R, st), E_SHAPE, "x3: odd W, pooled only")
    # residual: res_cstride < Cout, off the 4-grid, misaligned; with a pooled output (the planned entry point: the x3 one has no such argument)
    refused(x3r(ctypes.byref(desc(res_cstride=cout - 4)), P(x), None, P(filt), P(vec), None, None, P(res), P(y), P(sl), None, R, st), E_SHAPE,
            "x3: res_cstride < Cout")
    refused(x3r(ctypes.byref(desc(res_cstride=cout + 2)), P(x), None, P(filt), P(vec), None, None, P(res), P(y), P(sl), None, R, st), E_SHAPE,
            "x3: res_cstride % 4")
    refused(x3r(ctypes.byref(desc(res_cstride=cout + 8)), P(x), None, P(filt), P(vec), None, None, P(res, 4), P(y), P(sl), None, R, st), E_SHAPE,
            "x3: residual misaligned")
    dres = desc(res_cstride=cout + 8)
    assert PLAN[int(lib.shdr_conv2d_plan_f32(ctypes.byref(dres), 1))] == "x3"
    ws = torch.empty(4096, device="cuda", dtype=torch.uint8)
    refused(lib.shdr_conv2d_fwd_prepared_ranged_f32(ctypes.byref(dres), P(x), None, P(filt), P(vec), None, None, P(res), P(y), P(yp), P(ws), P(sl),
                                                    None, R, st), E_SHAPE, "planned x3: residual with a pooled output")
    assert K._conv2d_raw(x[:n * h * w * c].view(n, h, w, c), torch.zeros((3, 3, c, cout), device="cuda"), None, 1, None, 1.0, 0, None, None,
                         res[:n * h * w * (cout + 8)].view(n, h, w, cout + 8), 0, K.ALGO_AUTO, None, None, None, None, 0, None,
                         proj=torch.zeros((3, cout), device="cuda")) is None, "the wrapper forms no projected output of a layer with a residual"
    # projection: Cout != 64, proj without y_proj
    refused(x3p(ctypes.byref(desc(co=128)), P(x), None, P(filt), P(vec), None, None, P(vec), P(yj), None, None, P(sl), None, R, st), E_SHAPE,
            "x3: projection on Cout 128")
    refused(x3p(ctypes.byref(good), P(x), None, P(filt), P(vec), None, None, P(vec), None, P(y), None, P(sl), None, R, st), E_NULL, "x3: proj without y_proj")
    refused(x3p(ctypes.byref(good), P(x), None, P(filt), P(vec), None, None, P(vec, 4), P(yj), None, None, P(sl), None, R, st), E_SHAPE,
            "x3: projection map misaligned")
    # tanh is not compiled into the wide kernels: the predicate declines, the entry point refuses
    for f in ("act1", "act2"):
        dt = desc(**{f: C.ACT_TANH})
        assert lib.shdr_conv2d_x3_ok_f32(ctypes.byref(dt)) == 0
        refused(x3(ctypes.byref(dt), P(x), None, P(filt), P(vec), None, None, P(y), None, P(sl), None, R, st), E_SHAPE, "x3: tanh as " + f)
    # conv_x3n
    gn = desc(c1=16, co=16)
    assert lib.shdr_conv2d_x3n_ok_f32(ctypes.byref(gn)) == 1
    refused(x3n(ctypes.byref(gn), P(x, 4), None, P(filt), P(vec), None, None, None, P(y), None, P(sl), None, R, st), E_ALIGN, "x3n: x1 misaligned")
    refused(x3n(ctypes.byref(gn), P(x), None, P(filt), P(vec), None, None, None, P(y, 8), None, P(sl), None, R, st), E_ALIGN, "x3n: y misaligned")
    refused(x3n(ctypes.byref(gn), P(x), None, P(filt, 4), P(vec), None, None, None, P(y), None, P(sl), None, R, st), E_ALIGN, "x3n: filter misaligned")
    refused(x3n(ctypes.byref(gn), P(x), P(x), P(filt), P(vec), None, None, None, P(y), None, P(sl), P(sl), R, st), E_NULL, "x3n: x2 without C2")
    refused(x3n(ctypes.byref(desc(c1=16, c2=16, co=16)), P(x), None, P(filt), P(vec), None, None, None, P(y), None, P(sl), None, R, st), E_NULL,
            "x3n: C2 without x2")
    refused(x3n(ctypes.byref(gn), P(x), None, P(filt), P(vec), P(vec), None, None, P(y), None, P(sl), None, R, st), E_NULL, "x3n: scale without shift")
    refused(x3n(ctypes.byref(desc(c1=16, co=16, hh=15)), P(x), None, P(filt), P(vec), None, None, None, P(y), P(yp), P(sl), None, R, st), E_SHAPE,
            "x3n: odd H, pooled")
    refused(x3n(ctypes.byref(desc(c1=16, co=16, cv=3)), P(x), None, P(filt), P(vec), None, None, None, P(y), P(yp), P(sl), None, R, st), E_SHAPE,
            "x3n: pooled output of a narrow head")
    refused(x3n(ctypes.byref(desc(c1=16, co=16, res_cstride=12)), P(x), None, P(filt), P(vec), None, None, P(res), P(y), None, P(sl), None, R, st),
            E_SHAPE, "x3n: res_cstride < Cout")
    refused(x3n(ctypes.byref(desc(c1=16, c2=16, co=32, act1=C.ACT_TANH)), P(x), P(x), P(filt), P(vec), None, None, None, P(y), None, P(sl), P(sl), R, st),
            E_SHAPE, "x3n: tanh on a two-source layer")
    refused(x3n(ctypes.byref(desc(c1=16, co=32, act2=C.ACT_TANH)), P(x), None, P(filt), P(vec), None, None, None, P(y), None, P(sl), None, R, st),
            E_SHAPE, "x3n: tanh on 32 couts")
