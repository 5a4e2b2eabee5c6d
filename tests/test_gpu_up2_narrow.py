"""The narrow instantiations of the one-launch low-res form of the up-sampling 3x3 layers (csrc/up2_fused.hip at 16 and 32 output channels,
two and four patches per block) and the Dequantization-Net's `up` blocks on the low-res forms.

1. y and the range slot against the float64 model of tests/up2_narrow_ref.py, EXACTLY, between guard words: integer / dyadic operands make
   every sum of the GEMM and the fold exact in any order.  Every (Cin, Cout) pair on every grid with three epilogues; two grids leave
   waves of a block idle.
2. Random operands at scale 1, 1e-3 and 1e3: within 1e-5 of the maximum of the float64 oracle of the ideal layer and within 5e-6 of
   today's K.conv2d_up2 (the bars of tests/up2_fused_ref.py).
3. The 64-cout instantiation still has the bits of the two-launch form.
4. Determinism, the SHDR_NO_UP2_NARROW switch, refusals, the Dequantization-Net forward.
SHDR_X3_MIN_BLOCKS=1 takes the fill-the-chip thresholds of the paths compared against (speed only) out of the way."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as C
import up2_fused_ref as U
import up2_narrow_ref as R
from conftest import quantised_image, rel_err
from oracle import nets
from test_gpu_conv_x3_exact import E_SHAPE, LIMIT, SLOT_CONTENTS, Slot, dev, guarded_f32, same, slot_of
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


def fused_abi(K, lib, n, h, wd, cin, cout, x, xr, w, bias, act1, scale, shift, act2, what, preset=0.0):
    """one guarded call of shdr_conv2d_fwd_up2_fused_f32 without a projection; returns (y, range slot)"""
    d = descriptor(K, n, h, wd, cin, cout, act1, act2)
    assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(d))) == 1, what
    nprep = int(lib.shdr_conv2d_up2_fused_filter_elems_f32(ctypes.byref(d)))
    assert nprep > 0, what
    pbuf, prepared, pnum = guarded_f32((nprep,))
    assert lib.shdr_conv2d_up2_fused_prepare_filter_f32(ctypes.byref(d), P(w), P(prepared), K._stream()) == 0, lib.shdr_last_error()
    guards_intact(pbuf, pnum, what + " prepared filter")
    ybuf, y, ynum = guarded_f32((n, 2 * h, 2 * wd, cout))
    slot = Slot(preset)
    rc = lib.shdr_conv2d_fwd_up2_fused_f32(ctypes.byref(d), P(x), P(prepared), P(bias), P(scale), P(shift), None, None, P(y), P(xr), P(slot.view),
                                           K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    guards_intact(ybuf, ynum, what + " y")
    return y.cpu().numpy(), slot


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. exact operands
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", R.EXACT_CASES, ids=[o["name"] for o in R.EXACT_CASES])
def test_y_and_range_slot_exact(K, lib, o):
    r = R.exact_reference(o)
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift")}
    preset = (U.X.seed_of(o["name"]) % 4 == 1) * 1.0e6
    y, slot = fused_abi(K, lib, o["n"], o["h"], o["w"], o["cin"], o["cout"], dev(r["x"]), slot_of(r["xb"]), dev(r["w"]), opt["bias"], r["act1"],
                        opt["scale"], opt["shift"], r["act2"], o["name"], preset)
    same(y, r["y"], o["name"] + " y")
    slot.check(r["ymax"], o["name"])


@pytest.mark.parametrize("bound", [b for _, b in SLOT_CONTENTS], ids=[t for t, _ in SLOT_CONTENTS])
def test_unusual_slot_contents(K, lib, bound):
    """up2_fused_kernel's share of tests/test_gpu_conv_x3_exact.py::test_unusual_slot_contents: the smallest int-mode case under an empty
    slot, infinity, a NaN pattern, a word with the sign bit set, a bound that is no power of two and a large one"""
    o = R.EXACT_CASES[0]
    assert o["mode"] == "int" and o["epi"] == "none"
    r = R.exact_reference(o)
    _, y_ref, gemm, stencil = C.up2_lowres(r["x"], bound, r["w"])
    assert gemm < LIMIT and stencil < LIMIT, "%s: not exact by construction under the slot %r" % (o["name"], bound)
    y, slot = fused_abi(K, lib, o["n"], o["h"], o["w"], o["cin"], o["cout"], dev(r["x"]), slot_of(bound), dev(r["w"]), None, r["act1"], None, None,
                        r["act2"], o["name"])
    same(y, y_ref, o["name"] + " y")
    slot.check(float(np.abs(y_ref).max()), o["name"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. random operands: the oracle and today's path
# ---------------------------------------------------------------------------------------------------------------------------------
def layer_args(K, o, epi):
    if epi == "up":
        return (t32(o["x"]), t32(o["w"]), t32(o["bias"]), K.ACT_RELU, t32(o["scale"]), t32(o["shift"]), K.ACT_RELU)
    return (t32(o["x"]), t32(o["w"]), t32(o["bias"]), K.ACT_LRELU)


@pytest.mark.parametrize("epi", ["lrelu", "up"])
@pytest.mark.parametrize("pair, grid, xscale", R.RANDOM_CASES, ids=["%s_x%g" % (R.case_id(p, g), k) for p, g, k in R.RANDOM_CASES])
def test_random_operands(K, lib, monkeypatch, pair, grid, xscale, epi):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    o = R.random_operands(pair, grid, xscale)
    ref = R.oracle(o, epi)
    taken = []
    inner = K._conv2d_up2_fused

    def counted(*a, **kw):
        r = inner(*a, **kw)
        taken.append(r is not None)
        return r

    monkeypatch.setattr(K, "_conv2d_up2_fused", counted)
    with torch.no_grad():
        got = K.conv2d_up2(*layer_args(K, o, epi), lowres=True, one_launch=True)
        assert taken == [True], "the one-launch form did not take the layer"
        today = K.conv2d_up2(*layer_args(K, o, epi))
    assert taken == [True] and not torch.equal(got, today), "today's path did not run, or the new one did not"
    e_oracle, e_paths = U.rel(got.cpu().numpy(), ref), U.rel(got.cpu().numpy(), today.double().cpu().numpy())
    print("%s x%g %s: %.3g of the oracle's maximum (bar %g), %.3g of today's (bar %g)" % (R.case_id(pair, grid), xscale, epi, e_oracle, U.TOL, e_paths,
                                                                                          U.TOL_PATHS))
    assert tuple(got.shape) == ref.shape and e_oracle <= U.TOL and e_paths <= U.TOL_PATHS


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the 64-cout instantiation: the bits of the two-launch form
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", U.SHAPES, ids=[U.shape_id(s) for s in U.SHAPES])
def test_64_couts_keep_the_bits_of_the_two_launch_form(K, lib, monkeypatch, shape):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    o = U.random_operands(shape)
    args = (t32(o["x"]), t32(o["w"]), t32(o["bias"]), K.ACT_RELU, t32(o["scale"]), t32(o["shift"]), K.ACT_RELU)
    K.absmax_slot(args[0])
    with torch.no_grad():
        want = K._conv2d_up2_lowres(*args)
        got = K._conv2d_up2_fused(*args)
        through = K.conv2d_up2(*args, lowres=True, one_launch=True)                              # the wrapper takes the one-launch form first
    assert want is not None and got is not None
    assert torch.equal(got, want) and torch.equal(K._range_of(got), K._range_of(want)) and torch.equal(through, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", R.PAIRS, ids=["c%dto%d" % p for p in R.PAIRS])
def test_two_runs_agree_and_the_switch_gives_todays_bits(K, lib, monkeypatch, pair):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    grid = R.RANDOM_GRIDS[1]
    o = R.random_operands(pair, grid)
    d = descriptor(K, grid[0], grid[1], grid[2], pair[0], pair[1], K.ACT_LRELU)
    with torch.no_grad():
        a = K.conv2d_up2(*layer_args(K, o, "lrelu"), lowres=True, one_launch=True)
        b = K.conv2d_up2(*layer_args(K, o, "lrelu"), lowres=True, one_launch=True)
        today = K.conv2d_up2(*layer_args(K, o, "lrelu"))
        assert torch.equal(a, b) and not torch.equal(a, today)
        assert torch.equal(K._range_of(a), K._range_of(b))
        monkeypatch.setenv("SHDR_NO_UP2_NARROW", "1")
        assert not K.up2_narrow_enabled()
        assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(d))) == (1 if pair[1] == 64 else 0)      # the 64-cout form is older than the switch
        off = K.conv2d_up2(*layer_args(K, o, "lrelu"), lowres=True, one_launch=True)
        assert torch.equal(off, K.conv2d_up2(*layer_args(K, o, "lrelu"), lowres=True))     # without the keyword the wrapper is the parent's, switch or not
        # under the switch the wrapper is the one from before the narrow forms: the two-launch form where that takes the layer (64 couts:
        # the bits of the one-launch form), else the default call
        assert torch.equal(off, a if pair[1] == 64 else today)


def test_refusals(K, lib, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    n, h, wd = 1, 4, 5
    for cin, cout in R.PAIRS + [(96, 32), (128, 32)]:
        assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(descriptor(K, n, h, wd, cin, cout)))) == 1, (cin, cout)
    declined = dict(cout48=descriptor(K, n, h, wd, 64, 48), cin160=descriptor(K, n, h, wd, 160, 32), odd_h=descriptor(K, n, h, wd, 32, 16),
                    odd_w=descriptor(K, n, h, wd, 64, 32), tanh1=descriptor(K, n, h, wd, 32, 16, act1=C.ACT_TANH),
                    tanh2=descriptor(K, n, h, wd, 64, 32, act2=C.ACT_TANH), cin48=descriptor(K, n, h, wd, 48, 16),
                    cin96_cout16=descriptor(K, n, h, wd, 96, 16),            # four patches of 96 channels are past the LDS of a CU
                    cin32_cout64=descriptor(K, n, h, wd, 32, 64))            # the 64-cout form starts at 64 input channels
    declined["odd_h"].H = declined["odd_h"].Ho = 2 * h - 1
    declined["odd_w"].W = declined["odd_w"].Wo = 2 * wd - 1
    st = K._stream()
    x = torch.zeros((n * h * wd * 160,), device="cuda")
    prepared = torch.zeros((16 + 160 * 640 * 2,), device="cuda")
    vec = torch.zeros((3 * 64,), device="cuda")
    sl = slot_of(2.0)
    ybuf, y, _ = guarded_f32((n, 2 * h, 2 * wd, 64))
    jbuf, yj, _ = guarded_f32((n, 2 * h, 2 * wd, 3))
    rbuf = Slot(0.0)
    fwd = lib.shdr_conv2d_fwd_up2_fused_f32

    def refused(rc, what):
        assert rc == E_SHAPE, (what, rc, lib.shdr_last_error())
        for b in (ybuf, jbuf):
            untouched(b, what)
        rbuf.check(0.0, what)

    for what, d in declined.items():
        assert int(lib.shdr_conv2d_up2_fused_ok_f32(ctypes.byref(d))) == 0, what
        refused(fwd(ctypes.byref(d), P(x), P(prepared), None, None, None, None, None, P(y), P(sl), P(rbuf.view), st), "declined layer: " + what)
    for what in ("cout48", "cin160", "odd_h", "cin48", "cin96_cout16", "cin32_cout64"):
        assert int(lib.shdr_conv2d_up2_fused_filter_elems_f32(ctypes.byref(declined[what]))) == -1, what
        assert lib.shdr_conv2d_up2_fused_prepare_filter_f32(ctypes.byref(declined[what]), P(x), P(prepared), st) == E_SHAPE, what
    for cin, cout in ((32, 16), (64, 32)):                                       # a projection is the 64-cout form's
        d = descriptor(K, n, h, wd, cin, cout)
        refused(fwd(ctypes.byref(d), P(x), P(prepared), None, None, None, P(vec), P(yj), P(y), P(sl), P(rbuf.view), st), "proj with %d couts" % cout)
    # through the wrapper a layer the new entry declines is today's call, bit for bit; with a projection and narrow couts it is today's too
    rng = np.random.default_rng(12)
    with torch.no_grad():
        for what, (c1, cout, act1) in dict(cout48=(64, 48, K.ACT_LRELU), tanh=(32, 16, K.ACT_TANH), cin96_cout16=(96, 16, K.ACT_LRELU)).items():
            xs, w = t32(rng.normal(size=(1, 6, 7, c1))), t32(rng.normal(size=(3, 3, c1, cout)) / np.sqrt(9 * c1))
            assert torch.equal(K.conv2d_up2(xs, w, None, act1, lowres=True, one_launch=True), K.conv2d_up2(xs, w, None, act1)), what
        xs, w, proj = t32(rng.normal(size=(1, 6, 7, 32))), t32(rng.normal(size=(3, 3, 32, 16)) / np.sqrt(9 * 32)), t32(rng.normal(size=(3, 16)))
        got, today = K.conv2d_up2(xs, w, None, K.ACT_LRELU, proj=proj, lowres=True, one_launch=True), K.conv2d_up2(xs, w, None, K.ACT_LRELU, proj=proj)
        assert (got is None and today is None) or torch.equal(got, today)


def test_dequantization_net_forward_takes_the_new_path(shdr, K, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    p = nets.init_params(nets.deq_spec(), 21)
    m = shdr.dequantization_net.model().load_numpy(p)
    x = quantised_image(np.random.default_rng(1), (2, 64, 64, 3))
    calls = {"fused": [], "lowres": []}

    def counting(name):
        inner = getattr(K, "_conv2d_up2_" + name)

        def counted(xx, w, *a, **kw):
            r = inner(xx, w, *a, **kw)
            calls[name].append((tuple(w.shape[2:]), r is not None))
            return r
        return counted

    monkeypatch.setattr(K, "_conv2d_up2_fused", counting("fused"))
    monkeypatch.setattr(K, "_conv2d_up2_lowres", counting("lowres"))
    with torch.no_grad():
        y = m(t32(x), training=False).cpu().numpy()
    # u4 on the two-launch form (256 -> 128 is past one block), u3 on the 64-cout instantiation, u2 and u1 on the narrow ones
    assert calls["lowres"] == [((256, 128), True)]
    assert calls["fused"] == [((256, 128), False), ((128, 64), True), ((64, 32), True), ((32, 16), True)]
    assert rel_err(y, nets.deq_forward(p, x)) <= 1e-4                           # the bar of tests/test_gpu_nets.py
    monkeypatch.setenv("SHDR_NO_UP2_NARROW", "1")
    calls["fused"].clear()
    calls["lowres"].clear()
    with torch.no_grad():
        off = m(t32(x), training=False).cpu().numpy()
    assert calls == {"fused": [], "lowres": []} and rel_err(off, nets.deq_forward(p, x)) <= 1e-4
