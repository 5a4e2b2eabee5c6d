"""The up-sampling 3x3 layers with the channel mix at LOW resolution (csrc/up2_lowres.hip: shdr_conv2d_fwd_up2_lowres_f32 and its three
companions) against the float64 model of tests/conv_ref.py (up2_lowres), EXACTLY and element by element.

The model restates the two launches, not the ideal layer: launch A is conv_split of the low-res x with the filter restaged to
[1, 1, Cin, 9 Cout (+ pad)] -- all nine taps under ONE weight exponent S -- and launch B the bilinear stencil over the tap planes z.  The
operand is split at low resolution, before any blend, so all four operand modes of tests/test_gpu_conv_x3_exact.py (int / fx / fw / fxw)
run exactly through it.  Two preconditions are asserted on the reference before the kernel is called: the GEMM's sum of |terms| is below
2^24 units of the terms' lsb, and the stencil's sum A of |weight z| is below 2^24 units of lsb_z / 16 (every stencil weight is a multiple
of 1 / 16): every fp32 partial sum of both launches is then exact, in any order.  The epilogue is conv_ref.epilogue.

Per case, bit for bit with -0 mapped to +0: z read back from the CALLER'S workspace (all Cp columns, the padded ones +0), y, and the range
slot.  y, the whole workspace with its 256-byte tail slot, and the range slot sit between guard words; what lies in the workspace beyond
z must keep its sentinel, except the first word of the tail slot when the input arrives without a range.  The C ABI is called through
shdr._lib; one test goes through K.conv2d_up2(lowres=True).  SHDR_X3_MIN_BLOCKS=1 takes the fill-the-chip threshold of the GEMM's plan
(speed only) out of the way."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as C
from test_gpu_conv_x3_exact import LIMIT, E_SHAPE, E_ALIGN, E_NULL, Slot, bits32, dev, epilogue_operands, guarded_f32, operands, same, seed_of, slot_of
from test_gpu_wgrad_f32_exact import SENT32, P, guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

TAIL = 256                                                               # bytes of the workspace's tail slot (include/shdr.h)


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: low-res N x h x w, Cin -> Cout.  w from {1, 15, 16, 17, 33} (the 16-column strips, inactive lanes, both border taps), h from
# {1, 2, 3, 4, 5, 9, 17} (the walk unrolled by three, the seams of the 4-row segments these grids take), N 1 / 2 / 3, Cin 64 / 96 / 160 /
# 512 (2, 3, 5 and 16 chunks), Cout 64 / 128 / 192 / 256 / 512 (576 -> 640, 1152 -> 1280, 1728 -> 1792, 2304 and 4608 columns)
# ---------------------------------------------------------------------------------------------------------------------------------
def case(name, n, h, w, cin, cout, mode="int", epi="plain", **o):
    o.update(name=name, n=n, h=h, w=w, cin=cin, cout=cout, mode=mode, epi=epi)
    o.setdefault("ops", name)                                            # the name that seeds the operands (shared by the forms of one shape)
    o.setdefault("env", {})
    return pytest.param(o, id=name)


CASES = [
    case("ul_c64_64_1x1x1_int", 1, 1, 1, 64, 64),
    case("ul_c64_64_1x1x15_fx_relu", 1, 1, 15, 64, 64, "fx", "relu"),
    case("ul_c64_128_1x2x16_fw_lrelu", 1, 2, 16, 64, 128, "fw", "lrelu"),
    case("ul_c96_64_1x3x17_fxw_affine", 1, 3, 17, 96, 64, "fxw", "affine"),
    case("ul_c64_64_1x4x33_fx_act2", 1, 4, 33, 64, 64, "fx", "act2"),
    case("ul_c64_64_1x5x33_fx_nobias", 1, 5, 33, 64, 64, "fx", "nobias"),
    case("ul_c64_64_1x17x1_fw", 1, 17, 1, 64, 64, "fw"),
    case("ul_c96_128_2x9x15_fxw_act2", 2, 9, 15, 96, 128, "fxw", "act2"),
    case("ul_c64_192_3x4x17_int_lrelu", 3, 4, 17, 64, 192, "int", "lrelu"),
    case("ul_c96_192_1x5x16_fw_relu", 1, 5, 16, 96, 192, "fw", "relu"),
    case("ul_c160_256_1x17x15_fxw_affine", 1, 17, 15, 160, 256, "fxw", "affine", keep=0.5, kmax=1),
    case("ul_c160_64_2x3x33_fx_relu", 2, 3, 33, 160, 64, "fx", "relu", keep=0.5, kmax=1),
    case("ul_c512_512_1x5x16_fxw_act2", 1, 5, 16, 512, 512, "fxw", "act2", keep=0.25, kmax=1),
    case("ul_c512_64_3x2x1_int_nobias", 3, 2, 1, 512, 64, "int", "nobias"),
    # the rows of a segment, forced: each form against the model, not against another run
    case("ul_rows1_c160_256_1x17x15_fxw_affine", 1, 17, 15, 160, 256, "fxw", "affine", keep=0.5, kmax=1, ops="ul_c160_256_1x17x15_fxw_affine",
         env={"SHDR_UP2_LOWRES_ROWS": "1"}),
    case("ul_rows5_c160_256_1x17x15_fxw_affine", 1, 17, 15, 160, 256, "fxw", "affine", keep=0.5, kmax=1, ops="ul_c160_256_1x17x15_fxw_affine",
         env={"SHDR_UP2_LOWRES_ROWS": "5"}),
    case("ul_rows32_c160_256_1x17x15_fxw_affine", 1, 17, 15, 160, 256, "fxw", "affine", keep=0.5, kmax=1, ops="ul_c160_256_1x17x15_fxw_affine",
         env={"SHDR_UP2_LOWRES_ROWS": "32"}),
    # both paddings of the GEMM's columns: 1152 (nine 128-cout blocks) and 1280 (five 256-cout blocks)
    case("ul_pad128_c96_128_2x9x15_fxw_act2", 2, 9, 15, 96, 128, "fxw", "act2", ops="ul_c96_128_2x9x15_fxw_act2", pad=128,
         env={"SHDR_UP2_LOWRES_PAD": "128"}),
    case("ul_pad256_c96_128_2x9x15_fxw_act2", 2, 9, 15, 96, 128, "fxw", "act2", ops="ul_c96_128_2x9x15_fxw_act2", pad=256,
         env={"SHDR_UP2_LOWRES_PAD": "256"}),
]
RANGES_CASE = case("ul_ranges_c96_128_2x5x17_int_affine", 2, 5, 17, 96, 128, "int", "affine")
NAN_CASE = case("ul_nan_c64_64_1x5x17_int", 1, 5, 17, 64, 64)
WRAPPER_CASE = CASES[7]

_REF = {}


def reference(o):
    """everything of a case that needs no device, computed once per (operands, padding) and left unchanged"""
    key = (o["ops"], o.get("pad"), o["epi"])
    if key in _REF:
        return _REF[key]
    n, h, w, cin, cout = (o[f] for f in ("n", "h", "w", "cin", "cout"))
    x, xb, _, _, wt = operands(o["ops"], n, h, w, cin, 0, cout, 3, o["mode"], 1.0, o.get("keep", 1.0), o.get("kmax", 2))
    bias, act1, scale, shift, _, act2 = epilogue_operands(o["ops"], o["epi"], cout, (n, 2 * h, 2 * w))
    z, v, gemm, stencil = C.up2_lowres(x, xb, wt, o.get("pad"))
    assert gemm < LIMIT, "%s: GEMM sum |terms| / lsb = %.3g 2^24: the accumulator is not exact by construction" % (o["name"], gemm / LIMIT)
    assert stencil < LIMIT, "%s: stencil A / (lsb_z / 16) = %.3g 2^24: the pass is not exact by construction" % (o["name"], stencil / LIMIT)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v) and np.array_equal(z.astype(np.float32).astype(np.float64), z)
    y = C.epilogue(v if bias is None else v + bias, act1, scale, shift, None, act2)
    r = dict(x=x, xb=xb, w=wt, bias=bias, act1=act1, scale=scale, shift=shift, act2=act2, z=z.astype(np.float32), v=v, y=y,
             ymax=float(np.abs(y).max()), cp=z.shape[3], gemm=gemm / LIMIT, stencil=stencil / LIMIT)
    for a in (r["z"], r["y"]):
        a.setflags(write=False)
    _REF[key] = r
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# the guarded call
# ---------------------------------------------------------------------------------------------------------------------------------
def descriptor(K, n, h, w, cin, cout, act1=0, act2=0):
    d = K._conv_desc((n, 2 * h, 2 * w, cin), (3, 3, cin, cout), 1, 0, 1.0, None)
    d.act1, d.act2 = act1, act2
    d.algo = K._auto(K.ALGO_AUTO)
    d.y_cstride = cout
    d.prologue = K.PROLOGUE_BILINEAR2X
    return d


def prepare(K, lib, d, wd):
    prepared = torch.empty(int(lib.shdr_conv2d_up2_lowres_filter_elems_f32(ctypes.byref(d))), device="cuda")
    assert lib.shdr_conv2d_up2_lowres_prepare_filter_f32(ctypes.byref(d), P(wd), P(prepared), K._stream()) == 0, lib.shdr_last_error()
    return prepared


def run(K, lib, o, r, monkeypatch, ranges="declared", preset=None, x=None, check=True):
    """one call through the C ABI with every output between guards; returns (z, y) as they lie on the device"""
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    for name, value in o["env"].items():
        monkeypatch.setenv(name, value)
    n, h, w, cin, cout = (o[f] for f in ("n", "h", "w", "cin", "cout"))
    what = "%s (ranges %s)" % (o["name"], ranges)
    d = descriptor(K, n, h, w, cin, cout, r["act1"], r["act2"])
    assert int(lib.shdr_conv2d_up2_lowres_ok_f32(ctypes.byref(d))) == 1, what
    cp = C.up2_lowres_columns(cout, o.get("pad"))
    zbytes = n * h * w * cp * 4
    wsbytes = int(lib.shdr_conv2d_up2_lowres_workspace_bytes_f32(ctypes.byref(d)))
    assert cp == r["cp"] and wsbytes == (zbytes + 255) // 256 * 256 + TAIL, (what, cp, wsbytes)
    st = K._stream()
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() if x is not None else dev(r["x"])
    prepared = prepare(K, lib, d, dev(r["w"]))
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift")}
    xr = None
    if ranges == "declared":
        xr = slot_of(r["xb"])
    elif ranges == "measured":
        xr = slot_of(0.0)
        assert lib.shdr_absmax_f32(P(xd), xd.numel(), P(xr), st) == 0
    ybuf, y, ynum = guarded_f32((n, 2 * h, 2 * w, cout))
    wbuf, ws = guarded(wsbytes // 4)
    slot = Slot((seed_of(o["name"]) % 4 == 0) * 1.0e6 if preset is None else preset)
    rc = lib.shdr_conv2d_fwd_up2_lowres_f32(ctypes.byref(d), P(xd), P(prepared), P(opt["bias"]), P(opt["scale"]), P(opt["shift"]), P(y), P(ws),
                                            P(xr), P(slot.view), st)
    assert rc == 0, (what, rc, lib.shdr_last_error())
    guards_intact(ybuf, ynum, what + " y")
    guards_intact(wbuf, wsbytes // 4, what + " workspace")
    raw = ws.cpu().numpy()
    zgot = raw[:zbytes // 4].view(np.float32).reshape(n, h, w, cp)
    rest = raw[zbytes // 4:].view(np.uint32).copy()
    if ranges == "none":                                                 # the tail slot's first word: max |x|, measured below the ABI
        word = (wsbytes - TAIL - zbytes) // 4
        assert int(rest[word]) == bits32(np.abs(r["x"]).max()), what + ": the tail slot does not hold max |x|"
        rest[word] = SENT32
    assert (rest == SENT32).all(), what + ": the workspace was written beyond z"
    ygot = y.cpu().numpy()
    if check:
        same(zgot, r["z"], what + " z", "pixels")
        same(ygot, r["y"], what + " y")
        slot.check(r["ymax"], what)
    return zgot, ygot, slot


@pytest.mark.parametrize("o", CASES)
def test_up2_lowres_exact(K, lib, o, monkeypatch):
    run(K, lib, o, reference(o), monkeypatch, ranges="declared" if o["mode"] in ("fx", "fxw") else ("declared", "measured", "none")[seed_of(o["name"]) % 3])


def test_declared_measured_and_absent_ranges_agree_bit_for_bit(K, lib, monkeypatch):
    o = RANGES_CASE.values[0]
    r = reference(o)
    for preset in (0.0, 1.0e6):
        got = [run(K, lib, o, r, monkeypatch, ranges=ranges, preset=preset) for ranges in ("declared", "measured", "none")]
        for zg, yg, slot in got[1:]:
            assert np.array_equal(zg.view(np.uint32), got[0][0].view(np.uint32)) and np.array_equal(yg.view(np.uint32), got[0][1].view(np.uint32))
            assert torch.equal(slot.view.cpu(), got[0][2].view.cpu())
        assert bits32(got[0][2].view.cpu().numpy()) == max(bits32(r["ymax"]), bits32(preset))


@pytest.mark.parametrize("where", ["interior", "corner"])
def test_one_nan_reaches_its_footprint_and_nothing_else(K, lib, monkeypatch, where):
    """a NaN at low-res pixel (m, j) makes that pixel of z NaN in every column (NaN x 0 weights included) and y NaN on the hi-res rows
    2m - 2 .. 2m + 3 and columns 2j - 2 .. 2j + 3 (clipped), all channels: resize2x spreads it to 2m - 1 .. 2m + 2, the 3x3 taps by one
    more.  Every other element has the bits of the run without the NaN."""
    o = NAN_CASE.values[0]
    r = reference(o)
    n, h, w, cout = o["n"], o["h"], o["w"], o["cout"]
    m, j = (2, 8) if where == "interior" else (0, 0)
    z0, y0, _ = run(K, lib, o, r, monkeypatch)
    x = r["x"].astype(np.float32)
    x[0, m, j, 5] = np.nan
    z1, y1, _ = run(K, lib, o, r, monkeypatch, x=x, check=False)
    zn = r["z"].astype(np.float64)
    zn[0, m, j, :] = np.nan
    mask = np.isnan(C.up2_lowres_stencil(zn, cout)[0])
    hand = np.zeros((n, 2 * h, 2 * w, cout), dtype=bool)
    hand[0, max(2 * m - 2, 0):2 * m + 4, max(2 * j - 2, 0):2 * j + 4, :] = True
    assert np.array_equal(mask, hand), "the model's NaN footprint is not the one derived by hand"
    assert np.array_equal(np.isnan(z1), np.isnan(zn)), "z: the NaN pixel"
    same(np.where(np.isnan(zn), 0.0, z1), np.where(np.isnan(zn), 0.0, z0), "z away from the NaN pixel", "pixels")
    assert np.array_equal(np.isnan(y1), mask), "y: NaN mask differs from the model's at %d elements" % int((np.isnan(y1) != mask).sum())
    same(np.where(mask, 0.0, y1), np.where(mask, 0.0, y0), "y outside the NaN footprint")


# ---------------------------------------------------------------------------------------------------------------------------------
# the stencil pass alone on full-mantissa values
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 17, 64, 64), (2, 9, 15, 96, 128)], ids=["1x5x17_64_64", "2x9x15_96_128"])
def test_stencil_alone_on_gaussian_values(K, lib, monkeypatch, shape):
    """Gaussian x and w, no epilogue: y against the float64 stencil of the DEVICE'S OWN z.  Bar per element: |got - ref| <= 13 2^-24 A, A the
    stencil's sum of |weight z|: the pass is two multiplies and ten FMAs per output, each at most half an ulp of a partial sum, and every
    partial sum is <= A: 12 2^-24 A; the thirteenth absorbs second order."""
    n, h, w, cin, cout = shape
    rng = np.random.default_rng(seed_of("ul_gauss_%dx%dx%d_%d_%d" % shape))
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32)
    wt = (rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    o = dict(name="ul_gauss", n=n, h=h, w=w, cin=cin, cout=cout, env={})
    r = dict(x=x.astype(np.float64), xb=float(np.abs(x).max()), w=wt.astype(np.float64), bias=None, scale=None, shift=None, act1=0, act2=0,
             cp=C.up2_lowres_columns(cout))
    zgot, ygot, slot = run(K, lib, o, r, monkeypatch, ranges="measured", preset=0.0, check=False)
    ref, a = C.up2_lowres_stencil(zgot, cout)
    frac = np.abs(ygot.astype(np.float64) - ref) / (13 * 2.0 ** -24 * a)
    i = np.unravel_index(int(np.argmax(frac)), frac.shape)
    print("stencil alone %s: worst |got - ref| = %.4f of the bar 13 2^-24 A, at %s" % (shape, float(frac.max()), i))
    assert float(a.min()) > 0.0 and float(frac.max()) <= 1.0, (float(frac.max()), i, float(ygot[i]), float(ref[i]))
    slot.check(float(np.abs(ygot).max()), "stencil alone")


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python wrapper; refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_gives_the_bits_of_the_guarded_abi_call(K, lib, monkeypatch):
    o = WRAPPER_CASE.values[0]
    r = reference(o)
    _, ygot, _ = run(K, lib, o, r, monkeypatch)
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift")}
    with torch.no_grad():
        y = K.conv2d_up2(K.set_bound(dev(r["x"]), r["xb"]), dev(r["w"]), opt["bias"], r["act1"], opt["scale"], opt["shift"], r["act2"], lowres=True)
    same(y.cpu().numpy(), ygot, o["name"] + " through the wrapper")
    same(y.cpu().numpy(), r["y"], o["name"] + " through the wrapper, against the model")
    assert bits32(K._range_of(y).cpu().numpy()) == bits32(r["ymax"])


def test_refusals_leave_y_and_the_workspace_untouched(K, lib, monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    n, h, w, cin, cout = 1, 4, 5, 64, 64
    good = descriptor(K, n, h, w, cin, cout)
    assert int(lib.shdr_conv2d_up2_lowres_ok_f32(ctypes.byref(good))) == 1
    st = K._stream()
    x = torch.zeros((n * h * w * cin + 8,), device="cuda")
    wd = torch.zeros((3, 3, cin, cout), device="cuda")
    wd[0, 0, 0, 0] = 1.0
    nprep = int(lib.shdr_conv2d_up2_lowres_filter_elems_f32(ctypes.byref(good)))
    prepared = torch.zeros((nprep + 8,), device="cuda")
    assert lib.shdr_conv2d_up2_lowres_prepare_filter_f32(ctypes.byref(good), P(wd), P(prepared), st) == 0
    vec = torch.zeros((cout + 8,), device="cuda")
    sl = slot_of(2.0)
    ybuf, y, _ = guarded_f32((n, 2 * h, 2 * w, cout))
    wsbytes = int(lib.shdr_conv2d_up2_lowres_workspace_bytes_f32(ctypes.byref(good)))
    wbuf, ws = guarded(wsbytes // 4 + 4)
    pbuf, pv = guarded(nprep)
    rbuf = Slot(0.0)
    R = P(rbuf.view)
    fwd = lib.shdr_conv2d_fwd_up2_lowres_f32

    def refused(rc, code, what):
        assert rc == code, (what, rc, code, lib.shdr_last_error())
        for b in (ybuf, wbuf, pbuf):
            untouched(b, what)
        rbuf.check(0.0, what)

    g = ctypes.byref(good)
    # null pointers; scale without shift (and the reverse)
    refused(fwd(None, P(x), P(prepared), P(vec), None, None, P(y), P(ws), P(sl), R, st), E_NULL, "null descriptor")
    refused(fwd(g, None, P(prepared), P(vec), None, None, P(y), P(ws), P(sl), R, st), E_NULL, "null x")
    refused(fwd(g, P(x), None, P(vec), None, None, P(y), P(ws), P(sl), R, st), E_NULL, "null prepared filter")
    refused(fwd(g, P(x), P(prepared), P(vec), None, None, None, P(ws), P(sl), R, st), E_NULL, "null y")
    refused(fwd(g, P(x), P(prepared), P(vec), None, None, P(y), None, P(sl), R, st), E_NULL, "null workspace")
    refused(fwd(g, P(x), P(prepared), P(vec), P(vec), None, P(y), P(ws), P(sl), R, st), E_NULL, "scale without shift")
    refused(fwd(g, P(x), P(prepared), P(vec), None, P(vec), P(y), P(ws), P(sl), R, st), E_NULL, "shift without scale")
    # each of the seven pointers off the 16-byte grid
    refused(fwd(g, P(x, 4), P(prepared), P(vec), P(vec), P(vec), P(y), P(ws), P(sl), R, st), E_ALIGN, "x misaligned")
    refused(fwd(g, P(x), P(prepared, 8), P(vec), P(vec), P(vec), P(y), P(ws), P(sl), R, st), E_ALIGN, "prepared filter misaligned")
    refused(fwd(g, P(x), P(prepared), P(vec, 4), P(vec), P(vec), P(y), P(ws), P(sl), R, st), E_ALIGN, "bias misaligned")
    refused(fwd(g, P(x), P(prepared), P(vec), P(vec, 12), P(vec), P(y), P(ws), P(sl), R, st), E_ALIGN, "scale misaligned")
    refused(fwd(g, P(x), P(prepared), P(vec), P(vec), P(vec, 8), P(y), P(ws), P(sl), R, st), E_ALIGN, "shift misaligned")
    refused(fwd(g, P(x), P(prepared), P(vec), P(vec), P(vec), P(y, 4), P(ws), P(sl), R, st), E_ALIGN, "y misaligned")
    refused(fwd(g, P(x), P(prepared), P(vec), P(vec), P(vec), P(y), P(ws, 8), P(sl), R, st), E_ALIGN, "workspace misaligned")
    # layers the predicate declines
    declined = dict(cin32=descriptor(K, n, h, w, 32, cout), cout32=descriptor(K, n, h, w, cin, 32), odd_h=descriptor(K, n, h, w, cin, cout),
                    c2=descriptor(K, n, h, w, cin, cout), stride2=descriptor(K, n, h, w, cin, cout),
                    tanh1=descriptor(K, n, h, w, cin, cout, act1=C.ACT_TANH), tanh2=descriptor(K, n, h, w, cin, cout, act2=C.ACT_TANH))
    declined["odd_h"].H = declined["odd_h"].Ho = 2 * h - 1
    declined["c2"].C2 = 32
    declined["stride2"].stride, declined["stride2"].Ho, declined["stride2"].Wo = 2, h, w
    for what, d in declined.items():
        assert int(lib.shdr_conv2d_up2_lowres_ok_f32(ctypes.byref(d))) == 0, what
        refused(fwd(ctypes.byref(d), P(x), P(prepared), P(vec), None, None, P(y), P(ws), P(sl), R, st), E_SHAPE, "declined layer: " + what)
    # the companions
    d1 = descriptor(K, n, h, w, cin, cout)
    d1.KH = d1.KW = 1
    refused(lib.shdr_conv2d_up2_lowres_prepare_filter_f32(ctypes.byref(d1), P(wd), P(pv), st), E_SHAPE, "prepare_filter on a 1x1 filter")
    refused(lib.shdr_conv2d_up2_lowres_prepare_filter_f32(g, None, P(pv), st), E_NULL, "prepare_filter without a filter")
    for what, d in (("odd_h", declined["odd_h"]), ("cin48", descriptor(K, n, h, w, 48, cout)), ("cout32", declined["cout32"])):
        assert int(lib.shdr_conv2d_up2_lowres_filter_elems_f32(ctypes.byref(d))) == -1, what
    odd_w = descriptor(K, n, h, w, cin, cout)
    odd_w.W = odd_w.Wo = 2 * w - 1
    for what, d in (("odd_h", declined["odd_h"]), ("odd_w", odd_w)):
        assert int(lib.shdr_conv2d_up2_lowres_workspace_bytes_f32(ctypes.byref(d))) == -1, what
    assert int(lib.shdr_conv2d_up2_lowres_filter_elems_f32(None)) == -1 and int(lib.shdr_conv2d_up2_lowres_workspace_bytes_f32(None)) == -1
    # and the good call still goes through, into the same buffers
    assert fwd(g, P(x), P(prepared), P(vec), P(vec), P(vec), P(y), P(ws), P(sl), R, st) == 0, lib.shdr_last_error()
    torch.cuda.synchronize()
    assert not bool((y.view(torch.int32) == SENT32).any())
