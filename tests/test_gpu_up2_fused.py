"""The one-launch low-res form of the up-sampling 3x3 layers with 64 output channels (csrc/up2_fused.hip: shdr_conv2d_fwd_up2_fused_f32 and
its companions; the Hallucination-Net's u1 through K.conv2d_up2(proj=..., lowres=True)).

1. y without a projection is BIT-IDENTICAL to the two-launch form (K.conv2d_up2(lowres=True)), range slot included, for three epilogues.
2. y and the projected output against the float64 model of tests/up2_fused_ref.py, EXACTLY: integer / dyadic operands make every sum of
   the GEMM, the fold, the epilogue and the projection exact in any order (asserted on the reference, tests/test_up2_fused_ref.py).
3. Random operands: the projected output within 1e-5 of the maximum of the float64 oracle of the ideal layer and within 5e-6 of today's
   K.conv2d_up2(proj=...), also with inputs at 1e-3 and 1e3 scale.
4. Plumbing: determinism, the SHDR_NO_UP2_FUSED switch, refusals and fall-through, PROJECTED_LAUNCHES, the Hallucination-Net forward.
Every output of an ABI call and the range slot sit between guard words.  SHDR_X3_MIN_BLOCKS=1 takes the fill-the-chip thresholds of the
paths compared against (speed only) out of the way."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as C
import up2_fused_ref as U
from conftest import quantised_image, rel_err
from oracle import nets
from test_gpu_conv_x3_exact import E_NULL, E_SHAPE, Slot, bits32, dev, guarded_f32, same, seed_of, slot_of
from test_gpu_up2_lowres_exact import descriptor
from test_gpu_wgrad_f32_exact import P, guards_intact, untouched

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


def t32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def fused_abi(K, lib, shape, x, xr, w, bias, act1, scale, shift, act2, proj, want_y, what, preset=0.0):
    """one guarded call of shdr_conv2d_fwd_up2_fused_f32; returns (y or None, projected output or None, range slot)"""
    n, h, wd, cin = shape
    d = descriptor(K, n, h, wd, cin, U.COUT, act1, act2)
    assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(d))) == 1, what
    prepared = torch.empty(int(lib.shdr_conv2d_up2_fused_filter_elems_f32(ctypes.byref(d))), device="cuda")
    assert lib.shdr_conv2d_up2_fused_prepare_filter_f32(ctypes.byref(d), P(w), P(prepared), K._stream()) == 0, lib.shdr_last_error()
    ybuf = y = jbuf = yj = None
    if want_y:
        ybuf, y, ynum = guarded_f32((n, 2 * h, 2 * wd, U.COUT))
    if proj is not None:
        jbuf, yj, jnum = guarded_f32((n, 2 * h, 2 * wd, 3))
    slot = Slot(preset)
    rc = lib.shdr_conv2d_fwd_up2_fused_f32(ctypes.byref(d), P(x), P(prepared), P(bias), P(scale), P(shift), P(proj), P(yj), P(y), P(xr),
                                           P(slot.view), K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    if want_y:
        guards_intact(ybuf, ynum, what + " y")
    if proj is not None:
        guards_intact(jbuf, jnum, what + " projected output")
    return (None if y is None else y.cpu().numpy()), (None if yj is None else yj.cpu().numpy()), slot


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. y: the bits of the two-launch form
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epi", ["none", "bias_relu", "up"])
@pytest.mark.parametrize("shape", U.SHAPES, ids=[U.shape_id(s) for s in U.SHAPES])
def test_y_has_the_bits_of_the_two_launch_form(K, lib, monkeypatch, shape, epi):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    n, h, wd, cin = shape
    o = U.random_operands(shape)
    x, w = t32(o["x"]), t32(o["w"])
    bias = None if epi == "none" else t32(o["bias"])
    act1 = K.ACT_NONE if epi == "none" else K.ACT_RELU
    scale, shift, act2 = (t32(o["scale"]), t32(o["shift"]), K.ACT_RELU) if epi == "up" else (None, None, K.ACT_NONE)
    d = descriptor(K, n, h, wd, cin, U.COUT, act1, act2)
    assert int(lib.shdr_conv2d_up2_lowres_ok_f32(ctypes.byref(d))) == 1          # the reference below IS the two-launch form
    xr = K.absmax_slot(x)
    with torch.no_grad():
        want = K.conv2d_up2(x, w, bias, act1, scale, shift, act2, lowres=True)
    what = "%s %s" % (U.shape_id(shape), epi)
    y, _, slot = fused_abi(K, lib, shape, x, xr, w, bias, act1, scale, shift, act2, None, True, what)
    same(y, want.cpu().numpy(), what)
    slot.check(float(K._range_of(want).cpu()), what)
    with torch.no_grad():                                                        # and the wrapper's y-only form, range record included
        got = K._conv2d_up2_fused(x, w, bias, act1, scale, shift, act2)
    assert torch.equal(got, want) and torch.equal(K._range_of(got), K._range_of(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. exact operands: y and the projected output against the model, per element
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", U.EXACT_CASES, ids=[o["name"] for o in U.EXACT_CASES])
def test_projected_output_exact(K, lib, o):
    r = U.exact_reference(o)
    shape = (o["n"], o["h"], o["w"], o["cin"])
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift")}
    want_y = seed_of(o["name"]) % 2 == 0 or o["epi"] == "up"                     # both outputs, or the projected one alone
    preset = (seed_of(o["name"]) % 4 == 1) * 1.0e6
    y, yj, slot = fused_abi(K, lib, shape, dev(r["x"]), slot_of(r["xb"]), dev(r["w"]), opt["bias"], r["act1"], opt["scale"], opt["shift"], r["act2"],
                            dev(r["proj"]), want_y, o["name"], preset)
    same(yj, r["yj"], o["name"] + " projected output")
    if want_y:
        same(y, r["y"], o["name"] + " y")
        slot.check(r["ymax"], o["name"])
    else:
        slot.check(0.0, o["name"] + " (no y: the slot is not written)")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. random operands: the oracle and today's path
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, xscale", U.RANDOM_CASES, ids=["%s_x%g" % (U.shape_id(s), k) for s, k in U.RANDOM_CASES])
def test_projected_output_random_operands(K, lib, monkeypatch, shape, xscale):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    o = U.random_operands(shape, xscale)
    _, ref = U.oracle(o)
    args = (t32(o["x"]), t32(o["w"]), t32(o["bias"]), K.ACT_RELU, t32(o["scale"]), t32(o["shift"]), K.ACT_RELU)
    before = K.PROJECTED_LAUNCHES[0]
    with torch.no_grad():
        got = K.conv2d_up2(*args, proj=t32(o["proj"]), lowres=True)
        assert K.PROJECTED_LAUNCHES[0] == before + 1
        today = K.conv2d_up2(*args, proj=t32(o["proj"]))
    assert today is not None and not torch.equal(got, today), "today's path did not run, or the new one did not"
    e_oracle, e_paths = U.rel(got.cpu().numpy(), ref), U.rel(got.cpu().numpy(), today.double().cpu().numpy())
    print("%s x%g: %.3g of the oracle's maximum (bar %g), %.3g of today's (bar %g)" % (U.shape_id(shape), xscale, e_oracle, U.TOL, e_paths, U.TOL_PATHS))
    assert tuple(got.shape) == ref.shape and e_oracle <= U.TOL and e_paths <= U.TOL_PATHS


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
def up_args(K, o):
    return (t32(o["x"]), t32(o["w"]), t32(o["bias"]), K.ACT_RELU, t32(o["scale"]), t32(o["shift"]), K.ACT_RELU)


def test_two_runs_agree_and_the_switch_gives_todays_bits(K, lib, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    o = U.random_operands(U.SHAPES[6])
    proj = t32(o["proj"])
    with torch.no_grad():
        a = K.conv2d_up2(*up_args(K, o), proj=proj, lowres=True)
        b = K.conv2d_up2(*up_args(K, o), proj=proj, lowres=True)
        today = K.conv2d_up2(*up_args(K, o), proj=proj)
        assert torch.equal(a, b) and not torch.equal(a, today)
        monkeypatch.setenv("SHDR_NO_UP2_FUSED", "1")
        n, h, wd, cin = U.SHAPES[6]
        assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(descriptor(K, n, h, wd, cin, U.COUT)))) == 0
        before = K.PROJECTED_LAUNCHES[0]
        off = K.conv2d_up2(*up_args(K, o), proj=proj, lowres=True)
        assert torch.equal(off, today) and K.PROJECTED_LAUNCHES[0] == before + 1


def test_refusals_and_fall_through(K, lib, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    n, h, wd, cin = 1, 4, 5, 64
    good = descriptor(K, n, h, wd, cin, U.COUT)
    assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(good))) == 1
    declined = dict(cout128=descriptor(K, n, h, wd, cin, 128), tanh1=descriptor(K, n, h, wd, cin, U.COUT, act1=C.ACT_TANH),
                    tanh2=descriptor(K, n, h, wd, cin, U.COUT, act2=C.ACT_TANH), odd_h=descriptor(K, n, h, wd, cin, U.COUT),
                    odd_w=descriptor(K, n, h, wd, cin, U.COUT), cin160=descriptor(K, n, h, wd, 160, U.COUT), cin32=descriptor(K, n, h, wd, 32, U.COUT),
                    cin80=descriptor(K, n, h, wd, 80, U.COUT))
    declined["odd_h"].H = declined["odd_h"].Ho = 2 * h - 1
    declined["odd_w"].W = declined["odd_w"].Wo = 2 * wd - 1
    st = K._stream()
    x = torch.zeros((n * h * wd * 160,), device="cuda")
    prepared = torch.zeros((int(lib.shdr_conv2d_up2_lowres_filter_elems_f32(ctypes.byref(descriptor(K, n, h, wd, 160, 128)))),), device="cuda")
    vec = torch.zeros((3 * 128,), device="cuda")
    sl = slot_of(2.0)
    ybuf, y, _ = guarded_f32((n, 2 * h, 2 * wd, 128))
    jbuf, yj, _ = guarded_f32((n, 2 * h, 2 * wd, 3))
    rbuf = Slot(0.0)
    fwd = lib.shdr_conv2d_fwd_up2_fused_f32

    def refused(rc, code, what):
        assert rc == code, (what, rc, code, lib.shdr_last_error())
        for b in (ybuf, jbuf):
            untouched(b, what)
        rbuf.check(0.0, what)

    for what, d in declined.items():
        assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(d))) == 0, what
        refused(fwd(ctypes.byref(d), P(x), P(prepared), None, None, None, P(vec), P(yj), P(y), P(sl), P(rbuf.view), st), E_SHAPE, "declined layer: " + what)
    for what in ("cout128", "odd_h", "cin160", "cin80"):
        assert int(lib.shdr_conv2d_up2_fused_filter_elems_f32(ctypes.byref(declined[what]))) == -1, what
    g = ctypes.byref(good)
    refused(fwd(g, P(x), P(prepared), None, None, None, None, None, None, P(sl), P(rbuf.view), st), E_NULL, "neither output")
    refused(fwd(g, P(x), P(prepared), None, None, None, P(vec), None, P(y), P(sl), P(rbuf.view), st), E_NULL, "proj without y_proj")
    refused(fwd(g, P(x), P(prepared), None, None, None, None, P(yj), P(y), P(sl), P(rbuf.view), st), E_NULL, "y_proj without proj")
    refused(fwd(g, P(x), P(prepared), None, None, None, P(vec), P(yj), None, None, P(rbuf.view), st), E_NULL, "no range slot of the input")
    refused(fwd(g, P(x), P(prepared), None, P(vec), None, P(vec), P(yj), None, P(sl), P(rbuf.view), st), E_NULL, "scale without shift")
    # through the wrapper a layer the new entry declines is today's call, bit for bit (or today's None)
    rng = np.random.default_rng(11)
    with torch.no_grad():
        for what, (c1, cout, act1) in dict(cin160=(160, 64, K.ACT_RELU), tanh=(64, 64, K.ACT_TANH), cout128=(64, 128, K.ACT_RELU)).items():
            xs, w = t32(rng.normal(size=(1, 6, 7, c1))), t32(rng.normal(size=(3, 3, c1, cout)) / np.sqrt(9 * c1))
            proj = t32(rng.normal(size=(3, cout)))
            before = K.PROJECTED_LAUNCHES[0]
            got, today = K.conv2d_up2(xs, w, None, act1, proj=proj, lowres=True), K.conv2d_up2(xs, w, None, act1, proj=proj)
            assert (got is None and today is None) or torch.equal(got, today), what
            assert K.PROJECTED_LAUNCHES[0] - before == (0 if today is None else 2), what


def test_hallucination_net_forward_takes_the_new_path(shdr, K, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    p = nets.init_params(nets.hal_spec(), 23)
    m = shdr.hallucination_net.model().load_numpy(p)
    x = quantised_image(np.random.default_rng(3), (1, 64, 96, 3))
    taken = []
    inner = K._conv2d_up2_fused

    def counted(*a, **kw):
        r = inner(*a, **kw)
        taken.append(r is not None)
        return r

    monkeypatch.setattr(K, "_conv2d_up2_fused", counted)
    before = K.PROJECTED_LAUNCHES[0]
    with torch.no_grad():
        y = m(t32(x), training=False).cpu().numpy()
    assert taken == [True] and K.PROJECTED_LAUNCHES[0] - before == 2
    assert (y >= 0).all() and rel_err(y, nets.hal_forward(p, x)) <= 1e-4       # the bar of tests/test_gpu_nets.py
