"""Every fp16 tape kernel of csrc/elem_f16.hip (with its instantiations of csrc/nhwc_vec.h), element by element, against the float64
reference of tests/fp16_ref.py.

Two kinds of assertion, no tensor-scale bar ("fp16 tape ops"):

  exact     inputs built so that every intermediate is exactly representable (small integers, multiples of 2^-10): the fp32 / fp64
            partial sums are then exact in ANY order, so neither the atomics nor the grid shape can excuse a difference -- a missing,
            doubled or misrouted block changes the integer.  np.testing.assert_array_equal / torch.equal.
  half-ulp  |got - ref64| <= 0.5 ulp16(ref64) + k 2^-24 B per element: one fp16 rounding of the stored result plus k fp32 roundings
            on the longest path to it (counted from the kernel source, beside each case), B the bound of the magnitudes on that path.
            fp32 outputs have no fp16 term.  rsqrtf counts as 2 fp32 ulps = 4 units of 2^-24 (no accuracy table of the device
            library is at hand: assumed); elem_f16.hip calls no tanhf (the tanh gradient is g (1 - y^2) on the stored y) and is
            built with -ffp-contract=off, so a counted operation is one rounding.

The ops are called at _ops level with explicit operands (the relu mask of bn_bwd / act_bwd_bias is an INPUT here, nothing to excuse).
Shapes: the smallest that reach each branch; GS = (1, 264, 256, 64) is 540 672 16-byte vectors, just past the 2048-block cap of
shdr::stream_grid.  It is the LOOP DOMAIN of each kernel: where that is the smaller side of the op (the pools' outputs, the input
of resize2x) the other tensor is (1, 528, 512, 64), 35 MB.  Beyond those, the cases of test_*_large_* are the only ones above
10 MB (their branch is named beside each).
"""
import ctypes

import numpy as np
import pytest
import torch

import fp16_ref as F

pytestmark = pytest.mark.gpu
U = F.U32
GS = (1, 264, 256, 64)
SPATIAL = [(1, 1, 1), (1, 2, 2), (1, 2, 3), (2, 5, 7), (1, 7, 9), (1, 16, 12)]
CHANNELS = [8, 24, 40, 96, 136, 2048]      # one octet; odd octet count (octet_grid unit 3); 5; 12; gap's second block; bn OL = 256, PL = 1
RSQRT = 4                                   # rsqrtf: 2 fp32 ulps (assumed) in units of 2^-24
EPS = 1e-3


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


def hd(a):
    """host array -> fp16 device tensor (int8 data is widened on the device; every small integer is exact in fp16)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.int8:
        return torch.from_numpy(a).cuda().half()
    return torch.from_numpy(a.astype(np.float16)).cuda()


def fd(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def back(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape, dtype=np.int8)


def normal16(rng, shape, scale=1.0):
    return (rng.normal(size=shape) * scale).astype(np.float16)


def assert_bar(got, ref, k, B, out16=True, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bar = k * U * np.broadcast_to(np.asarray(B, dtype=np.float64), ref.shape)
    if out16:
        bar = bar + 0.5 * F.ulp16(ref)
    err = np.abs(got - ref)
    bad = ~(err <= bar)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bar, 1e-300), 0.0)), ref.shape)
        raise AssertionError("%s: %d of %d elements over the bar; worst at %s: got %r, reference %r, |err| %.4g, bar %.4g"
                             % (what, int(bad.sum()), ref.size, i, got[i], ref[i], err[i], bar[i]))


def assert_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.astype(np.float64), want.astype(np.float64), err_msg=what)


def assert_equal_dev(got, want_int8, what=""):
    """exact comparison of a large fp16 result with a host-computed small-integer expectation (widened on the device)"""
    want = torch.from_numpy(np.ascontiguousarray(want_int8)).cuda()
    assert tuple(got.shape) == tuple(want.shape), what
    assert want.dtype == torch.int8 and torch.equal(got.float(), want.float()), what


# ---- casts / packing -------------------------------------------------------------------------------------------------------
SPECIAL = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, -(1.0 + 2.0 ** -11),   # exact ties
                    65504.0, 65519.9, 65520.0, -65520.0, 1.0e5, -3.0e38,                                                       # round to infinity
                    2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 3 * 2.0 ** -25, 1.5 * 2.0 ** -24,     # subnormal results
                    2.0 ** -25 + 2.0 ** -40, 1.0e-8, 6.0e-8, 1.0e-6, -3.1e-5, 2.0 ** -126], dtype=np.float32)


def cast_inputs(n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=n) * 10.0 ** rng.uniform(-9, 5.5, size=n)).astype(np.float32)
    x[:SPECIAL.size] = SPECIAL
    return x


@pytest.mark.parametrize("n", [SPECIAL.size, 540672 + 77], ids=["special", "grid_stride"])
def test_cast_f32_to_f16_bit_exact(K, n):
    """round to nearest even, ties, results in the fp16 subnormal range, overflow to infinity -- NumPy's astype(float16)"""
    x = cast_inputs(n, 1)
    got = back(K.to_half(fd(x)))
    assert got.dtype == np.float16
    np.testing.assert_array_equal(got.view(np.uint16), F.cast_f16(x).view(np.uint16))


def test_cast_f16_to_f32_bit_exact(K):
    """every finite fp16 bit pattern (subnormals included), ten times over: 655 360 elements, past the 2048-block cap"""
    bits = np.arange(65536, dtype=np.uint16)
    h = np.tile(bits[np.isfinite(bits.view(np.float16))], 10).view(np.float16)
    got = back(K.to_float(torch.from_numpy(h).cuda()))
    assert got.dtype == np.float32 and h.size > 2048 * 256
    np.testing.assert_array_equal(got.view(np.uint32), h.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("npix,cin,cout", [(SPECIAL.size, 1, 8), (35, 3, 8), (35, 5, 16), (9, 8, 8), (2048 * 256 // 8 + 3, 3, 8)])
def test_pad_channels_h_bit_exact(K, npix, cin, cout):
    x = cast_inputs(npix * cin, 2).reshape(1, npix, 1, cin)
    got = back(K.pad_channels_h(fd(x), cout))
    np.testing.assert_array_equal(got.view(np.uint16), F.pad_channels(F.cast_f16(x), cout).view(np.uint16))


PACK_SHAPES = [(1, 1, 1), (2, 5, 7), (1, 16, 12)]


@pytest.mark.parametrize("nsrc,oc", [(1, 8), (2, 8), (3, 16), (4, 16), (2, 24), (4, 40)])
@pytest.mark.parametrize("nhw", PACK_SHAPES, ids=str)
def test_pack3_bit_exact(K, nhw, nsrc, oc):
    """2 to 4 sources (and one), multiples of 2^-10 in [-1, 1]: exact in fp16"""
    rng = np.random.default_rng(nsrc * 100 + oc)
    srcs = [rng.integers(-1024, 1025, size=nhw + (3,)) / 1024.0 for _ in range(nsrc)]
    got = back(K.pack3([fd(s) for s in srcs], oc, dtype=torch.float16))
    assert got.dtype == np.float16
    assert_equal(got, F.pack3(srcs, oc))


@pytest.mark.parametrize("nout,c", [(1, 8), (2, 8), (3, 16), (4, 16), (1, 24), (4, 40)])
@pytest.mark.parametrize("nhw", PACK_SHAPES, ids=str)
def test_unpack3_bit_exact(K, nhw, nout, c):
    rng = np.random.default_rng(nout * 100 + c)
    y = (rng.integers(-1024, 1025, size=nhw + (c,)) / 1024.0).astype(np.float16)
    outs = K.unpack3(hd(y), nout)
    want = F.unpack3(y, nout)
    assert len(outs) == nout
    for o, w in zip(outs, want):
        assert o.dtype == torch.float32
        assert_equal(back(o), w)


def test_pack3_unpack3_grid_stride_bit_exact(K):
    """270 336 pixels x 2 octets (pack3) and 67 584 pixels x 12 values (unpack3): past the 2048-block cap"""
    rng = np.random.default_rng(6)
    srcs = [rng.integers(-1024, 1025, size=(1, 264, 1024, 3)) / 1024.0 for _ in range(3)]
    assert_equal(back(K.pack3([fd(s) for s in srcs], 16, dtype=torch.float16)), F.pack3(srcs, 16))
    y = (rng.integers(-1024, 1025, size=(1, 264, 256, 16)) / 1024.0).astype(np.float16)
    for o, w in zip(K.unpack3(hd(y), 4), F.unpack3(y, 4)):
        assert_equal(back(o), w)


@pytest.mark.parametrize("nhw", PACK_SHAPES + [(1, 264, 256)], ids=str)
@pytest.mark.parametrize("oc", [8, 16])
def test_pack3_unpack3_vgg_half_ulp(K, nhw, oc):
    rng = np.random.default_rng(nhw[1] + oc)
    x = rng.random(nhw + (3,)).astype(np.float32) * 1.25
    got = back(K.vgg_preprocess(fd(x), oc, dtype=torch.float16))
    # k = 3: x * 255, the fp32 rounding of the mean constant, the subtraction; B = |x| 255 + mean
    assert_bar(got, F.pack3([x], oc, vgg=True), 3, F.pad_channels(F.pack3_vgg_abs(x), oc), what="pack3 vgg")
    assert not got[..., 3:].any()
    g = normal16(rng, nhw + (oc,))
    dx = back(K.vgg_preprocess_bwd(hd(g)))
    # k = 1: (float)g * 255 (fp32 output: no fp16 term); B = |g| 255
    assert dx.dtype == np.float32
    assert_bar(dx, F.unpack3(g, 1, vgg=True)[0], 1, np.abs(g.astype(np.float64))[..., 2::-1] * 255.0, out16=False, what="unpack3 vgg")


# ---- activation backward + bias gradient -----------------------------------------------------------------------------------
def bias_case(rng, shape):
    """dy: an integer in [-4, 4] plus a per-channel offset in [-2, 2] (a channel mix-up changes the sum), y in {-1, 0, 1},
    db starts from a non-zero integer vector"""
    c = shape[-1]
    dy = (ints(rng, shape, -4, 4) + ((np.arange(c) % 5) - 2).astype(np.int8)).astype(np.int8)
    y = ints(rng, shape, -1, 1)
    start = ((np.arange(c) * 7) % 11 - 5).astype(np.int64)
    start[start == 0] = 3
    npix = dy.size // c
    assert 6 * npix + 5 < 2 ** 24            # every partial sum of |dy| (any order, any grouping) is an exact fp32 integer
    return dy, y, start


def run_bias_exact(K, shape, act, want_db, seed):
    rng = np.random.default_rng(seed)
    dy, y, start = bias_case(rng, shape)
    c = shape[-1]
    dyd, yd = hd(dy), hd(y)
    out = fd(start) if want_db else None
    dz, db = K.act_bwd_bias_h(dyd, yd if act else None, act, want_db, out=out)
    want_dz = dy if act == F.ACT_NONE else np.where(y > 0, dy, 0).astype(np.int8)
    if act == F.ACT_NONE:
        assert dz.data_ptr() == dyd.data_ptr()                 # dz == dy: nothing is written
    else:
        assert dz.dtype == torch.float16
        assert_equal_dev(dz, want_dz, "dz")
    if want_db:
        want = start + want_dz.reshape(-1, c).sum(axis=0, dtype=np.int64)
        assert db is out
        assert_equal(back(db), want, "db = start + sum dz")
    else:
        assert db is None


@pytest.mark.parametrize("act", [F.ACT_NONE, F.ACT_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("nhw", SPATIAL, ids=str)
def test_act_bwd_bias_exact(K, nhw, c, act):
    run_bias_exact(K, nhw + (c,), act, True, c + nhw[1])
    if act:
        run_bias_exact(K, nhw + (c,), act, False, c + nhw[2])


BIAS_LARGE = [
    ((1, 264, 256, 64), "grid-stride: 540 672 vectors, 256-block cap with db (four vectors in flight, atomics), 2048 without"),
    ((1, 300, 301, 24), "2^18 < nvec = 270 900 < 2^22, odd octet count: grid 258, four vectors in flight + tail, ends in atomics"),
    ((4, 512, 512, 32), "nvec = 2^22: partial rows + col_fold over 2048 rows"),
    ((1, 1366, 1024, 24), "nvec = 4 196 352, odd octet count: octet_grid rounds to 2049 > kBiasMaxBlocks, re-grid to 1026 rows"),
]


# (ACT_NONE without db launches nothing: dz is dy)
@pytest.mark.parametrize("act,want_db", [(F.ACT_NONE, True), (F.ACT_RELU, True), (F.ACT_RELU, False)], ids=["none_db", "relu_db", "relu_no_db"])
@pytest.mark.parametrize("shape", [s for s, _ in BIAS_LARGE], ids=str)
def test_act_bwd_bias_large_exact(K, shape, act, want_db):
    run_bias_exact(K, shape, act, want_db, shape[1])


def test_act_bwd_bias_large_atomics_without_workspace(shdr, K):
    """db without a workspace at nvec = 2^23: the 512-block cap, every block ends in global atomics (a host that passes ws = NULL;
    _ops always passes one) -- straight through the C ABI"""
    shape = (8, 512, 512, 32)
    rng = np.random.default_rng(23)
    c = shape[-1]
    dy = (ints(rng, shape, -4, 4) + ((np.arange(c) % 5) - 2).astype(np.int8)).astype(np.int8)
    npix = dy.size // c
    assert npix * (c // 8) == 2 ** 23 and 6 * npix + 5 < 2 ** 24
    start = (np.arange(c) % 7 + 1).astype(np.int64)
    dyd, db = hd(dy), fd(start)
    lib = shdr._lib.load()
    rc = lib.shdr_act_bwd_bias_f16(K._ptr(dyd), None, None, K._ptr(db), None, npix, c, F.ACT_NONE, K._stream())
    assert rc == 0, lib.shdr_last_error()
    assert_equal(back(db), start + dy.reshape(-1, c).sum(axis=0, dtype=np.int64))


@pytest.mark.parametrize("act", [F.ACT_LRELU, F.ACT_TANH], ids=["lrelu", "tanh"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 5, 7, 24), (1, 7, 9, 40), (1, 16, 12, 136), GS], ids=str)
def test_act_bwd_bias_lrelu_tanh_half_ulp(K, shape, act):
    rng = np.random.default_rng(shape[3] + act)
    c = shape[-1]
    dy = normal16(rng, shape)
    y = np.tanh(rng.normal(size=shape)).astype(np.float16) if act == F.ACT_TANH else normal16(rng, shape)
    start = rng.normal(size=c).astype(np.float32)
    dz, db = K.act_bwd_bias_h(hd(dy), hd(y), act, True, out=fd(start))
    ref = F.act_grad(dy, y, act)
    g, yy = np.abs(dy.astype(np.float64)), y.astype(np.float64)
    if act == F.ACT_TANH:
        kz, Bz = 3, g * (1.0 + yy * yy)        # y * y, 1 - yy, g * (..)
    else:
        kz, Bz = 2, g                          # the fp32 rounding of the constant 0.1, the product
    assert_bar(back(dz), ref, kz, Bz, what="dz")
    # db, from the launch geometry of shdr_act_bwd_bias_f16 (nvec < 2^22: no partial rows, 256-block cap): a thread adds its
    # ceil(nvec / threads) terms (kz roundings each), the ceil(256 / O) threads of a block that share an octet meet in LDS atomics, the
    # blocks in global atomics onto the starting value; B = sum |term| + |start|
    o = c // 8
    nvec = dy.size // 8
    assert nvec < 2 ** 22
    unit = o // np.gcd(o, 256)
    grid = -(-min(-(-nvec // 256), 256) // unit) * unit
    kdb = kz + -(-nvec // (grid * 256)) + -(-256 // o) + grid
    assert_bar(back(db), start.astype(np.float64) + ref.reshape(-1, c).sum(axis=0), kdb,
               Bz.reshape(-1, c).sum(axis=0) + np.abs(start), out16=False, what="db")
    dz2, none = K.act_bwd_bias_h(hd(dy), hd(y), act, False)
    assert none is None and torch.equal(dz2, dz)


# ---- add -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [False, True], ids=["add", "add_relu"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 2, 3, 24), (2, 5, 7, 40), GS], ids=str)
def test_add_exact(K, shape, relu):
    rng = np.random.default_rng(shape[3])
    a, b = ints(rng, shape, -60, 60), ints(rng, shape, -60, 60)
    want = a.astype(np.int16) + b
    want = np.maximum(want, 0) if relu else want
    assert_equal_dev(K.add(hd(a), hd(b), relu=relu), want.astype(np.int8))


# ---- pools -----------------------------------------------------------------------------------------------------------------------
def domain(shape, scale_h=1, scale_w=1):
    n, h, w, c = shape
    return (n, h * scale_h, w * scale_w, c)


POOL_SHAPES = [s + (c,) for s in SPATIAL for c in (8, 24)]


@pytest.mark.parametrize("shape", [s for s in POOL_SHAPES if s[1] >= 2 and s[2] >= 2] + [domain(GS, 2, 2)], ids=str)
def test_avgpool2_exact(K, shape):
    """x an integer in [-8, 8]: the four-sum and the quarter are exact.  Odd sizes: the last row / column takes no part forward
    and must come back as zero.  (The large case makes the OUTPUT the grid-stride size.)"""
    rng = np.random.default_rng(shape[1] * shape[2])
    x = ints(rng, shape, -8, 8)
    y = K.avgpool2(hd(x))
    assert_equal(back(y), F.avgpool2(x))
    n, h, w, c = shape
    xs = shape if h * w * c < 10 ** 6 else GS                     # backward: the INPUT gradient is the loop domain
    dy = ints(rng, (xs[0], xs[1] // 2, xs[2] // 2, c), -8, 8)
    dx = K.avgpool2_bwd(hd(dy), xs)
    assert tuple(dx.shape) == tuple(xs)
    assert_equal(back(dx), F.avgpool2_bwd(dy, xs))


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 4, 6, 24), (1, 16, 12, 8), domain(GS, 2, 2)], ids=str)
def test_maxpool2_exact(K, shape):
    """values from {0, 1, 2}: most windows tie; the gradient goes to the first maximum in row-major order"""
    rng = np.random.default_rng(shape[1])
    x = ints(rng, shape, 0, 2)
    xd = hd(x)
    y = K.maxpool2(xd)
    assert_equal(back(y), F.maxpool2(x))
    dy = ints(rng, tuple(y.shape), -8, 8)
    dy[dy == 0] = 5                                               # a non-zero gradient everywhere: a wrong winner always shows
    assert_equal(back(K.maxpool2_bwd(xd, hd(dy))), F.maxpool2_bwd(x, dy))


@pytest.mark.parametrize("shape", POOL_SHAPES + [GS, domain(GS, 2, 2)], ids=str)
def test_maxpool3s2_exact(K, shape):
    """MaxPool2D(3, 2, SAME) at 1 x 1, 2 x 3 and odd sizes; tied windows; overlapping windows sum their (integer) gradients.
    The forward loops over the OUTPUT, the backward over the input: GS is the grid-stride size of the backward, its double that of
    the forward (whose backward is then the GS case again and is not repeated)"""
    rng = np.random.default_rng(shape[1] + shape[3])
    x = ints(rng, shape, 0, 2)
    xd = hd(x)
    y = K.maxpool3s2(xd)
    if shape[1] > GS[1]:
        assert tuple(y.shape) == GS
        return assert_equal(back(y), F.ops.max_pool(x.astype(np.float32), 3, 2))      # (small integers: float32 states them exactly)
    assert_equal(back(y), F.maxpool3s2(x))
    dy = ints(rng, tuple(y.shape), -8, 8)
    dy[dy == 0] = 5
    assert_equal(back(K.maxpool3s2_bwd(xd, y, hd(dy))), F.maxpool3s2_bwd(x, dy))


@pytest.mark.parametrize("shape", POOL_SHAPES + [GS], ids=str)
def test_upsample_zero2_exact(K, shape):
    rng = np.random.default_rng(shape[2])
    n, h, w, c = shape
    dy = normal16(rng, (n, (h + 1) // 2, (w + 1) // 2, c))
    got = back(K.upsample_zero2(hd(dy), shape))
    np.testing.assert_array_equal(got.view(np.uint16), F.upsample_zero2(dy, shape).astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("shape", [s for s in POOL_SHAPES if s[1] >= 2 and s[2] >= 2] + [domain(GS, 2, 2)], ids=str)
def test_avgpool2_half_ulp(K, shape):
    rng = np.random.default_rng(shape[1])
    x = normal16(rng, shape)
    # k = 3: (a + b), (c + d), their sum; the quarter is exact.  B = avgpool2(|x|) x 4 (the partial sums are not yet quartered)
    assert_bar(back(K.avgpool2(hd(x))), F.avgpool2(x), 3, 4.0 * F.abs_bound("avgpool2", x), what="avgpool2")


# ---- resize ----------------------------------------------------------------------------------------------------------------------
RESIZE_SHAPES = [(1, 1, 1, 8), (1, 1, 6, 8), (1, 6, 1, 24), (1, 2, 3, 8), (2, 5, 7, 24), (1, 7, 9, 8), (1, 16, 12, 40), GS]


@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=str)
def test_resize2x_half_ulp(K, shape):
    rng = np.random.default_rng(shape[1] * 3 + shape[2])
    x = normal16(rng, shape)
    got = back(K.resize2x(hd(x)))
    # k = 6: two nested lerps a + (b - a) w of three operations each.  The difference b - a is bounded by |a| + |b| <= 4 lerp(|a|, |b|)
    # for w in {1/4, 3/4}: B = 4 resize2x(|x|)
    assert_bar(got, F.resize2x(x), 6, 4.0 * F.abs_bound("resize2x", x), what="resize2x")
    if shape[1] == 1 and shape[2] == 1:                        # all clamped taps coincide: the input, bit for bit
        assert_equal(got, np.broadcast_to(x, (1, 2, 2, shape[3])))


@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=str)
def test_resize2x_bwd_half_ulp(K, shape):
    rng = np.random.default_rng(shape[1] * 5 + shape[2])
    n, h, w, c = shape
    dy = normal16(rng, (n, 2 * h, 2 * w, c))
    got = back(K.resize2x_bwd(hd(dy), shape))
    # k = 17: up to 4 x 4 taps, each one product (the tap weight yw * xw is exact) and one addition onto the running sum, which
    # resize2x_bwd(|dy|) bounds
    assert_bar(got, F.resize2x_bwd(dy, shape), 17, F.abs_bound("resize2x_bwd", dy, shape), what="resize2x_bwd")


# ---- global average pool -----------------------------------------------------------------------------------------------------------
GAP_SHAPES = [(1, 1, 1), (1, 2, 2), (2, 5, 7), (1, 7, 9), (1, 16, 12), (3, 67, 1), (1, 20, 13)]      # HW = 1, 4 (< 16), 35, 63, 192, 67, 260


@pytest.mark.parametrize("c", [8, 24, 136, 2048])
@pytest.mark.parametrize("nhw", GAP_SHAPES, ids=str)
def test_gap_exact_sums(K, nhw, c):
    """sums of integers in [-8, 8] + a per-channel offset are exact in fp32 in any order; the mean is one correctly rounded
    division of that exact sum by HW: half an fp32 ulp from the exact quotient (the kernel used to multiply by the rounded
    reciprocal: 1.41 ulp at HW = 63)"""
    rng = np.random.default_rng(c + nhw[1])
    shape = nhw + (c,)
    x = (ints(rng, shape, -8, 8) + ((np.arange(c) % 5) - 2).astype(np.int8)).astype(np.int8)
    hw = nhw[1] * nhw[2]
    assert 10 * hw < 2 ** 24
    s = x.reshape(nhw[0], hw, c).sum(axis=1, dtype=np.int64)
    y = back(K.global_avg_pool(hd(x)))
    assert y.dtype == np.float32 and y.shape == (nhw[0], c)
    want = s / float(hw)
    assert (np.abs(y - want) <= 0.5 * F.ulp32(want)).all(), (np.abs(y - want) / F.ulp32(want)).max()
    assert_equal(y[s == 0], 0.0 * s[s == 0])
    if hw & (hw - 1) == 0:                                      # a power of two: the quotient is exact
        assert_equal(y, want)


@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 5, 7, 24), (1, 67, 1, 136), GS], ids=str)
def test_gap_and_gap_bwd_half_ulp(K, shape):
    rng = np.random.default_rng(shape[1])
    n, h, w, c = shape
    x = normal16(rng, shape)
    # k = ceil(HW / 16) additions per thread + 3 to join its four accumulators + 16 across the pixel lanes + the division;
    # fp32 output; B = mean |x|
    assert_bar(back(K.global_avg_pool(hd(x))), F.gap(x), -(-h * w // 16) + 20, F.abs_bound("gap", x), out16=False, what="gap")
    dy = rng.normal(size=(n, c)).astype(np.float32)
    dx = K.gap_bwd(fd(dy), shape, dtype=torch.float16)
    # k = 2: the reciprocal of HW and the product; B = |dy| / HW
    assert_bar(back(dx), F.gap_bwd(dy, shape), 2, F.abs_bound("gap_bwd", dy, shape), what="gap_bwd")


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------------
def bn_stats_raw(shdr, K, xd):
    """shdr_bn_stats_f16 with a workspace of our own: (sum x, sum x^2) as the kernels left them, mean, var"""
    lib = shdr._lib.load()
    c = xd.shape[-1]
    ws = K._bn_ws(c, xd.device)
    mean, var = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    rc = lib.shdr_bn_stats_f16(K._ptr(xd), K._ptr(ws), K._ptr(mean), K._ptr(var), None, None, xd.numel() // c, c, 0.99, K._stream())
    assert rc == 0, lib.shdr_last_error()
    return back(ws[:2 * c]).reshape(2, c), back(mean), back(var)


def bn_int_case(rng, shape):
    c = shape[-1]
    x = (ints(rng, shape, -7, 7) + ((np.arange(c) % 3) - 1).astype(np.int8)).astype(np.int8)      # in [-8, 8]
    # the fp32 partial sums run over at most 32 pixels (64 each at most), the rest is double: exact
    assert 32 * 64 < 2 ** 24 and 64 * (x.size // c) < 2 ** 53
    x2 = x.reshape(-1, c).astype(np.int32)
    return x, x2.sum(axis=0, dtype=np.int64), (x2 * x2).sum(axis=0, dtype=np.int64)


# pixels per stride of the capped grid (1024 blocks x PL): 16.1 and 16.02.  The statistics pass (mode 0) therefore runs its 8-wide loop
# twice and ends in the ragged 1-wide tail; the backward reduction (mode 1, no 8-wide loop) runs the 4-wide loop four times + the tail
BN_LARGE = [((1, 129, 128, 2048), "OL = 256, PL = 1, 1032 blocks capped at SHDR_BN_MAX_BLOCKS; 16 512 pixels"),
            ((1, 725, 724, 64), "PL = 32, 1026 blocks capped at 1024; 524 900 pixels, stride 32 768")]
# statistics only: 21 609 pixels = 21.1 strides of the capped grid -- 8-wide twice, then the 4-wide loop once, then the 1-wide tail
# (small shapes reach the 4-wide loop of mode 0 too, e.g. (1, 16, 12, 136): 12 strides; this one does with the block cap in force)
BN_STATS_4WIDE = (1, 147, 147, 2048)


@pytest.mark.parametrize("shape", [s + (c,) for s in SPATIAL for c in (8, 24, 136)] + [(2, 5, 7, 2048), GS] + [s for s, _ in BN_LARGE] + [BN_STATS_4WIDE],
                         ids=str)
def test_bn_stats_exact(shdr, K, shape):
    rng = np.random.default_rng(shape[1] + shape[3])
    x, s1, s2 = bn_int_case(rng, shape)
    npix = x.size // shape[-1]
    xd = hd(x)
    sums, mean, var = bn_stats_raw(shdr, K, xd)
    assert_equal(sums[0], s1, "sum x")
    assert_equal(sums[1], s2, "sum x^2")
    mu = s1 / float(npix)
    v = np.maximum(s2 / float(npix) - mu * mu, 0.0)
    assert (np.abs(mean - mu) <= F.ulp32(mu)).all() and (np.abs(var - v) <= F.ulp32(v)).all()
    # the wrapper: same statistics, and the moving ones (Keras momentum 0.99, unbiased variance)
    mm, mv = torch.full((shape[-1],), 2.0, device="cuda"), torch.full((shape[-1],), 3.0, device="cuda")
    m2, v2 = K.bn_stats(xd, mm, mv, 0.99)
    assert_equal(back(m2), mean)
    assert_equal(back(v2), var)
    unb = v * npix / (npix - 1) if npix > 1 else v
    # moving = old * 0.99 + new * (1 - 0.99) in fp32: the two constants, two products, one sum, the cast of `new`
    assert_bar(back(mm), 2.0 * 0.99 + mu * 0.01, 6, 2.0 + np.abs(mu), out16=False, what="moving mean")
    assert_bar(back(mv), 3.0 * 0.99 + unb * 0.01, 6, 3.0 + np.abs(unb), out16=False, what="moving variance")


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 2, 3, 24), (2, 5, 7, 40), (1, 16, 12, 136)], ids=str)
def test_bn_stats_half_ulp_inputs(K, shape):
    """fp16 data that is no integer: the fp32 partial sums round"""
    rng = np.random.default_rng(shape[3])
    x = normal16(rng, shape, 3.0) + np.float16(1.5)
    mean, var = K.bn_stats(hd(x))
    mu, v = F.bn_stats(x)
    a1, a2 = np.abs(x.astype(np.float64)).mean(axis=(0, 1, 2)), (x.astype(np.float64) ** 2).mean(axis=(0, 1, 2))
    # a run of at most 32 fp32 additions (+ the square) before the double accumulators, the division and the cast
    assert_bar(back(mean), mu, 34, a1, out16=False, what="mean")
    assert_bar(back(var), v, 36, a2 + mu * mu, out16=False, what="var")


def bn_params(rng, c):
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    beta = rng.normal(0, 0.3, c).astype(np.float32)
    return gamma, beta


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 2, 3, 24), (2, 5, 7, 40), (1, 7, 9, 96), (1, 16, 12, 136), (1, 2, 2, 2048), GS], ids=str)
def test_bn_train_apply_half_ulp(K, shape, relu):
    rng = np.random.default_rng(shape[3] + relu)
    c = shape[-1]
    x, s1, s2 = bn_int_case(rng, shape)
    npix = x.size // c
    mu = s1 / float(npix)
    mean = mu.astype(np.float32)                                          # the expected fp32 statistics, derived from the exact sums
    var = np.maximum(s2 / float(npix) - mu * mu, 0.0).astype(np.float32)
    gamma, beta = bn_params(rng, c)
    y = K.bn_train_apply(hd(x), fd(mean), fd(var), fd(gamma), fd(beta), EPS, relu)
    ref = F.bn_apply(x, mean, var, gamma, beta, EPS, relu)
    # k = 10: the cast of eps, var + eps, rsqrtf (4), * gamma, x - mean, * k0, + beta; B = (|x| + |mean|) |gamma| rstd + |beta|
    rstd = 1.0 / np.sqrt(var.astype(np.float64) + EPS)
    B = (np.abs(x.astype(np.float64)) + np.abs(mean)) * gamma * rstd + np.abs(beta)
    assert_bar(back(y), ref, 6 + RSQRT, B, what="bn_train_apply")


def run_bn_bwd(K, shape, masked, seed, chunks=1):
    """integer dy, x, y_relu and an integer-valued `mean` operand: sum dy' and sum dy' (x - mean) are exact integers, so dbeta is
    exact and the workspace sums can be read back; dgamma and dx carry rsqrtf and are held to their bars"""
    rng = np.random.default_rng(seed)
    c = shape[-1]
    npix = int(np.prod(shape[:3]))
    dy = (ints(rng, shape, -4, 4) + ((np.arange(c) % 3) - 1).astype(np.int8)).astype(np.int8)
    x = ints(rng, shape, -8, 8)
    yr = ints(rng, shape, -1, 1) if masked else None
    mean = ((np.arange(c) % 5) - 2).astype(np.float32)
    var = rng.uniform(0.5, 30.0, c).astype(np.float32)        # rstd <= 1.42: |dx| stays below 2100, far from the fp16 maximum
    gamma, _ = bn_params(rng, c)
    g0, b0 = ((np.arange(c) % 7) - 3).astype(np.float32), ((np.arange(c) % 9) - 4).astype(np.float32)
    assert 5 * 10 * 32 < 2 ** 24 and 5 * npix + 4 < 2 ** 24 and 50 * npix < 2 ** 53      # the fp32 runs, the fp32 dbeta, the double sums
    gm = dy if yr is None else np.where(yr > 0, dy, 0).astype(np.int8)
    s1 = gm.reshape(-1, c).sum(axis=0, dtype=np.int64)
    s2 = (gm.reshape(-1, c).astype(np.int32) * (x.reshape(-1, c).astype(np.int32) - mean.astype(np.int32))).sum(axis=0, dtype=np.int64)
    a1 = np.abs(gm.reshape(-1, c)).sum(axis=0, dtype=np.int64)
    a2 = (np.abs(gm.reshape(-1, c).astype(np.int32)) * np.abs(x.reshape(-1, c).astype(np.int32) - mean.astype(np.int32))).sum(axis=0, dtype=np.int64)
    dyd, xd, yd = hd(dy), hd(x), (hd(yr) if masked else None)
    dgamma, dbeta = fd(g0), fd(b0)
    dx, dg, db = K.bn_bwd(dyd, xd, yd, fd(mean), fd(var), fd(gamma), EPS, dgamma_out=dgamma, dbeta_out=dbeta)
    assert dg is dgamma and db is dbeta and dx.dtype == torch.float16
    assert_equal(back(db), b0 + s1, "dbeta = start + sum dy'")
    rstd = 1.0 / np.sqrt(var.astype(np.float64) + EPS)
    # dgamma: cast of eps, var + eps, rsqrtf (4), the cast of the double product, the accumulation: k = 8
    assert_bar(back(dg), g0 + s2 * rstd, 4 + RSQRT, np.abs(s2) * rstd + np.abs(g0), out16=False, what="dgamma")
    # dx = k0 (g - k1 - xh k2): rstd 6 (eps, +, rsqrtf); k0 = gamma rstd 7; k1 1; k2 = (float)(S2 / n) rstd 8; xh = (x - mean) rstd 8;
    # xh k2 17; g - k1 2; the difference 18; the product 26.  With data that is no integer the fp32 runs of S1 / S2 add up to 22 more:
    # k = 48 for every case.  B = |gamma| rstd (|g| + mean |dy'| + (|x| + |mean|) rstd mean(|dy'| |x - mean|) rstd)
    got = back(dx).reshape(-1, c)
    k0 = gamma.astype(np.float64) * rstd
    for idx in np.array_split(np.arange(npix), chunks):
        sl = slice(idx[0], idx[-1] + 1)
        g = gm.reshape(-1, c)[sl].astype(np.float64)
        xc = x.reshape(-1, c)[sl].astype(np.float64) - mean
        ref = k0 * (g - s1 / float(npix) - xc * rstd * (s2 / float(npix)) * rstd)
        B = k0 * (np.abs(g) + a1 / float(npix) + (np.abs(xc) * rstd) * (a2 / float(npix)) * rstd)
        assert_bar(got[sl], ref, 48, B, what="dx rows %d.." % idx[0])
    return dy, x, yr, mean, var, gamma, s1, s2


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "relu_mask"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (1, 2, 3, 24), (2, 5, 7, 40), (1, 7, 9, 96), (1, 16, 12, 136), (1, 2, 2, 2048), GS], ids=str)
def test_bn_bwd_integer_sums(K, shape, masked):
    dy, x, yr, mean, var, gamma, s1, s2 = run_bn_bwd(K, shape, masked, shape[3] + masked, chunks=4 if shape == GS else 1)
    if shape[1] <= 7:                 # the whole-array reference agrees with the chunked form used above
        dx, dgam, dbet = F.bn_bwd(dy, x, yr, mean, var, gamma, EPS)
        np.testing.assert_allclose(dbet, s1, atol=1e-9)
        np.testing.assert_allclose(dgam, s2 / np.sqrt(var.astype(np.float64) + EPS), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("shape", [s for s, _ in BN_LARGE], ids=str)
def test_bn_bwd_large(K, shape):
    run_bn_bwd(K, shape, True, shape[1], chunks=16)


@pytest.mark.parametrize("shape", [(1, 2, 3, 24), (2, 5, 7, 40), (1, 16, 12, 136)], ids=str)
def test_bn_bwd_half_ulp_general_inputs(K, shape):
    """fp16 data that is no integer, the batch statistics of x as mean / var: the float64 autograd-pinned reference"""
    rng = np.random.default_rng(shape[3] + 1)
    c = shape[-1]
    x, dy = normal16(rng, shape, 2.0) + np.float16(0.5), normal16(rng, shape)
    yr = normal16(rng, shape)
    mu, v = F.bn_stats(x)
    mean, var = mu.astype(np.float32), v.astype(np.float32)
    gamma, _ = bn_params(rng, c)
    dx, dg, db = K.bn_bwd(hd(dy), hd(x), hd(yr), fd(mean), fd(var), fd(gamma), EPS)
    rdx, rdg, rdb = F.bn_bwd(dy, x, yr, mean, var, gamma, EPS)
    adx, adg, adb = F.bn_bwd(dy, x, yr, mean, var, gamma, EPS, absolute=True)
    assert_bar(back(dx), rdx, 48, adx, what="dx")
    # the sums: runs of at most 32 fp32 additions of terms with up to 2 roundings, then double; rsqrtf chain 6, cast, accumulation
    assert_bar(back(db), rdb, 36, adb, out16=False, what="dbeta")
    assert_bar(back(dg), rdg, 44, adg, out16=False, what="dgamma")


# ---- Linearization-Net front end -----------------------------------------------------------------------------------------------------
FRONT_SHAPES = [(1, 2, 2), (1, 2, 3), (2, 5, 7), (1, 7, 9), (1, 16, 12), (1, 211, 209)]      # the last: 345 groups of six blocks > the 342 cap


def front_images(rng, nhw):
    """multiples of 2^-10 (every bin centre, bin edge and 0 / 1 occur: all arithmetic exact) and the 8-bit law k / 255"""
    a = rng.integers(0, 1025, size=nhw + (3,)) / 1024.0
    m = min(a.size, 33)
    a.reshape(-1)[:m] = rng.permutation(33)[:m] / 32.0
    b = np.round(rng.random(nhw + (3,)) * 255.0) / 255.0
    return [("dyadic", np.clip(a, 0.0, 1.0).astype(np.float32)), ("8bit", b.astype(np.float32))]


@pytest.mark.parametrize("nhw", FRONT_SHAPES, ids=str)
def test_lin_frontend_half_ulp(K, nhw):
    rng = np.random.default_rng(nhw[1] * 7 + nhw[2])
    for name, img in front_images(rng, nhw):
        f = back(K.lin_frontend(fd(img), 96, dtype=torch.float16))
        assert f.dtype == np.float16 and f.shape == nhw + (96,)
        ref = F.lin_frontend(img)
        # image channels: the cast alone (k = 0).  sobel: (a + 2b + c) - (d + 2e + f), the doublings exact: k = 5, B = sum |tap| |img|.
        # histogram: x - centre, * B, 1 - (..): k = 3, B = 2
        k = np.array([0] * 3 + [5] * 6 + [3] * 84 + [0] * 3, dtype=np.float64)
        assert_bar(f, ref, 1, k * F.lin_frontend_abs(img), what="lin_frontend " + name)
        assert not f[..., 93:].any()
        if name == "dyadic":          # exact arithmetic: the correctly rounded fp16 of the reference, bit for bit
            assert_equal(f, ref.astype(np.float16), "lin_frontend dyadic")


@pytest.mark.parametrize("nhw", FRONT_SHAPES[:-1] + [(1, 419, 418)], ids=str)
def test_lin_frontend_bwd(K, nhw):
    """(1, 419, 418): 525 426 elements, past the 2048-block cap"""
    rng = np.random.default_rng(nhw[1] * 11 + nhw[2])
    for name, img in front_images(rng, nhw):
        big = nhw[1] > 100
        dF = ints(rng, nhw + (96,), -8, 8) if big else normal16(rng, nhw + (96,))
        got = back(K.lin_frontend_bwd(fd(img), hd(dF)))
        assert got.dtype == np.float32
        ref = F.lin_frontend_bwd(img, dF)
        # k = 42: at most 6 live bins (the slope product +-B g is exact: one addition each) and the 3 x 3 neighbourhood, each position
        # two products, their sum and the accumulation; fp32 output; B = the same sums over magnitudes
        assert_bar(got, ref, 42, F.lin_frontend_bwd(img, dF, absolute=True), out16=False, what="lin_frontend_bwd " + name)
        if big:                       # integer gradients, integer weights: exact
            assert_equal(got, ref)
            break


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5
SENTINEL = 1234.0


class Refusal:
    def __init__(self, shdr, K):
        self.lib, self.K = shdr._lib.load(), K
        self.out = []

    def buf(self, n, dtype=torch.float16):
        t = torch.full((n + 16,), SENTINEL, device="cuda", dtype=dtype)
        self.out.append(t)
        return t

    def p(self, t, offset=0):
        return ctypes.c_void_p(t.data_ptr() + offset)

    def refused(self, code, fn, *args):
        rc = getattr(self.lib, fn)(*args, self.K._stream())
        torch.cuda.synchronize()
        assert rc == code, (fn, rc, self.lib.shdr_last_error())
        for t in self.out:
            assert bool((t == SENTINEL).all()), fn + ": a refused call wrote to its output"


@pytest.fixture
def refusal(shdr, K):
    return Refusal(shdr, K)


def test_refusals_nhwc_family(refusal):
    r = refusal
    x = torch.ones(2 * 6 * 6 * 16 + 16, device="cuda", dtype=torch.float16)
    y = r.buf(2 * 12 * 12 * 16)
    for fn in ("shdr_avgpool2_fwd_f16", "shdr_maxpool2_fwd_f16", "shdr_maxpool3s2_fwd_f16", "shdr_resize2x_fwd_f16", "shdr_avgpool2_bwd_f16",
               "shdr_resize2x_bwd_f16", "shdr_upsample_zero2_f16"):
        r.refused(E_ALIGN, fn, r.p(x), r.p(y), 2, 6, 6, 12)                   # C % 8 != 0
        r.refused(E_ALIGN, fn, r.p(x, 8), r.p(y), 2, 6, 6, 8)                 # a pointer offset by 8 bytes
        r.refused(E_ALIGN, fn, r.p(x), r.p(y, 8), 2, 6, 6, 8)
    r.refused(E_SHAPE, "shdr_maxpool2_fwd_f16", r.p(x), r.p(y), 2, 5, 6, 8)   # odd H
    r.refused(E_SHAPE, "shdr_maxpool2_fwd_f16", r.p(x), r.p(y), 2, 6, 5, 8)
    r.refused(E_SHAPE, "shdr_maxpool2_bwd_f16", r.p(x), r.p(x), r.p(y), 2, 5, 6, 8)
    r.refused(E_ALIGN, "shdr_maxpool2_bwd_f16", r.p(x), r.p(x), r.p(y), 2, 6, 6, 12)
    r.refused(E_ALIGN, "shdr_maxpool3s2_bwd_f16", r.p(x), r.p(x), r.p(x), r.p(y), 2, 6, 6, 12)
    r.refused(E_ALIGN, "shdr_maxpool3s2_bwd_f16", r.p(x), r.p(x), r.p(x), r.p(y, 8), 2, 6, 6, 8)
    yf = r.buf(64, torch.float32)
    r.refused(E_ALIGN, "shdr_gap_fwd_f16", r.p(x), r.p(yf), 2, 36, 12)
    r.refused(E_ALIGN, "shdr_gap_fwd_f16", r.p(x, 8), r.p(yf), 2, 36, 8)
    r.refused(E_ALIGN, "shdr_gap_bwd_f16", r.p(yf), r.p(y), 2, 36, 12)
    r.refused(E_ALIGN, "shdr_gap_bwd_f16", r.p(yf, 8), r.p(y), 2, 36, 8)     # dy is read as 16-byte float4s
    r.refused(E_ALIGN, "shdr_gap_bwd_f16", r.p(yf), r.p(y, 8), 2, 36, 8)


def test_refusals_act_bwd_bias_and_add(refusal):
    r = refusal
    x = torch.ones(4 * 16 + 16, device="cuda", dtype=torch.float16)
    dz, db, ws = r.buf(4 * 16), r.buf(16, torch.float32), r.buf(2048 * 16, torch.float32)
    f = "shdr_act_bwd_bias_f16"
    r.refused(E_SHAPE, f, r.p(x), r.p(x), r.p(dz), r.p(db), r.p(ws), 4, 12, 1)             # C % 8 != 0
    r.refused(E_ALIGN, f, r.p(x, 8), r.p(x), r.p(dz), r.p(db), r.p(ws), 4, 8, 1)          # a pointer offset by 8 bytes
    r.refused(E_ALIGN, f, r.p(x), r.p(x), r.p(dz, 8), r.p(db), r.p(ws), 4, 8, 1)
    for act in (1, 2, 3):
        r.refused(E_NULL, f, r.p(x), None, r.p(dz), r.p(db), r.p(ws), 4, 8, act)          # an activation but no y
    r.refused(E_NULL, f, r.p(x), r.p(x), None, r.p(db), r.p(ws), 4, 8, 1)
    y = r.buf(64)
    r.refused(E_SHAPE, "shdr_add_f16", r.p(x), r.p(x), r.p(y), 12, 0)
    r.refused(E_ALIGN, "shdr_add_f16", r.p(x, 8), r.p(x), r.p(y), 16, 0)
    r.refused(E_ALIGN, "shdr_add_f16", r.p(x), r.p(x), r.p(y, 8), 16, 1)


def test_refusals_batchnorm(refusal, K):
    r = refusal
    c = 12
    x = torch.ones(64 * 16, device="cuda", dtype=torch.float16)
    v = torch.ones(16, device="cuda")
    mean, var, y = r.buf(16, torch.float32), r.buf(16, torch.float32), r.buf(64 * 16)
    ws = K._bn_ws(16, x.device)
    r.refused(E_SHAPE, "shdr_bn_stats_f16", r.p(x), r.p(ws), r.p(mean), r.p(var), None, None, 64, c, 0.99)       # C % 8 != 0
    r.refused(E_NULL, "shdr_bn_stats_f16", r.p(x), r.p(ws), r.p(mean), r.p(var), r.p(mean), None, 64, 8, 0.99)   # moving stats come in pairs
    r.refused(E_SHAPE, "shdr_bn_train_apply_f16", r.p(x), r.p(v), r.p(v), r.p(v), r.p(v), r.p(y), 64, c, EPS, 1)
    r.refused(E_SHAPE, "shdr_bn_bwd_f16", r.p(x), r.p(x), None, r.p(v), r.p(v), r.p(v), r.p(ws), r.p(mean), r.p(var), r.p(y), 64, c, EPS)
    # a pointer offset by 8 bytes: every tensor the kernels move in 16-byte vectors (the fp16 maps, and `mean` of the backward reduction)
    r.refused(E_ALIGN, "shdr_bn_stats_f16", r.p(x, 8), r.p(ws), r.p(mean), r.p(var), None, None, 63, 8, 0.99)
    r.refused(E_ALIGN, "shdr_bn_train_apply_f16", r.p(x, 8), r.p(v), r.p(v), r.p(v), r.p(v), r.p(y), 63, 8, EPS, 1)
    r.refused(E_ALIGN, "shdr_bn_train_apply_f16", r.p(x), r.p(v), r.p(v), r.p(v), r.p(v), r.p(y, 8), 63, 8, EPS, 1)
    bwd = [r.p(x), r.p(x), r.p(x), r.p(v), r.p(v), r.p(v), r.p(ws), r.p(mean), r.p(var), r.p(y)]
    for i, off in ((0, r.p(x, 8)), (1, r.p(x, 8)), (2, r.p(x, 8)), (3, r.p(v, 8)), (9, r.p(y, 8))):
        r.refused(E_ALIGN, "shdr_bn_bwd_f16", *(bwd[:i] + [off] + bwd[i + 1:]), 63, 8, EPS)


def test_refusals_front_end_and_packing(refusal):
    r = refusal
    img = torch.rand(2 * 4 * 4 * 3 + 8, device="cuda")
    y = r.buf(2 * 4 * 4 * 104)
    f = "shdr_lin_frontend_fwd_f16"
    r.refused(E_SHAPE, f, r.p(img), r.p(y), 2, 4, 4, 104)                     # a multiple of 8 above 93 that is not the 96-channel layout
    r.refused(E_SHAPE, f, r.p(img), r.p(y), 2, 4, 4, 100)
    r.refused(E_SHAPE, f, r.p(img), r.p(y), 2, 1, 4, 96)
    r.refused(E_ALIGN, f, r.p(img), r.p(y, 8), 2, 4, 4, 96)
    g = r.buf(2 * 4 * 4 * 3, torch.float32)
    r.refused(E_SHAPE, "shdr_lin_frontend_bwd_f16", r.p(img), r.p(y), r.p(g), 2, 4, 4, 88)
    p = "shdr_pack3_f16"
    r.refused(E_SHAPE, p, r.p(img), r.p(img), None, None, 2, r.p(y), 8, 32, 1)            # the VGG preprocessing takes one source
    r.refused(E_SHAPE, p, r.p(img), None, None, None, 1, r.p(y), 12, 32, 0)               # out_channels % 8 != 0
    r.refused(E_SHAPE, p, r.p(img), r.p(img), r.p(img), None, 3, r.p(y), 8, 32, 0)        # 9 channels do not fit 8
    r.refused(E_NULL, p, r.p(img), None, None, None, 2, r.p(y), 8, 32, 0)                 # a missing source
    r.refused(E_ALIGN, p, r.p(img), None, None, None, 1, r.p(y, 8), 8, 32, 0)
    r.refused(E_SHAPE, "shdr_unpack3_f16", r.p(y), r.p(g), r.p(g), r.p(g), None, 3, 8, 32, 0)
    r.refused(E_NULL, "shdr_unpack3_f16", r.p(y), r.p(g), None, None, None, 2, 8, 32, 0)
    h = r.buf(64)
    r.refused(E_NULL, "shdr_cast_f32_to_f16", r.p(img), r.p(h), 0)
    r.refused(E_SHAPE, "shdr_pad_channels_f32_to_f16", r.p(img), r.p(h), 8, 3, 2)
