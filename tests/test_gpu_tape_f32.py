"""Every fp32 tape kernel of csrc/bwd.hip, pool.hip (both with the channel-vector kernels of nhwc_vec.h), glue.hip, crf.hip, finetune.hip
(+ soft_hist_bwd / lin_frontend_bwd), element by element, against the float64 reference of tests/tape_ref.py.

Two kinds of assertion, no tensor-scale bar:

  exact    inputs built so that every intermediate is exactly representable (small integers, multiples of 2^-10, dyadic weights): the
           fp32 / fp64 partial sums are then exact in ANY order, so neither the atomics nor the grid shape can excuse a difference.
           np.testing.assert_array_equal / torch.equal.
  counted  |got - ref64| <= k 2^-24 B per element: k fp32 roundings on the longest path to the element (counted from the kernel
           source, beside each case), B the bound of the magnitudes on that path.  These translation units are NOT built with
           -ffp-contract=off: a fused multiply-add rounds once where the count assumes two, so the unfused count stays an upper
           bound.  fp32 sums that end in atomics over random inputs: (n - 1) 2^-24 sum |terms| (tape_ref.sum_bar).
           Device-library calls carry ASSUMED bounds (no accuracy table of the device library is at hand), marked below; every
           such test prints the worst distance it observed ("observed ...": DESIGN.md 4.2 records them).  Division and sqrtf are
           taken as correctly rounded (HIP's default for fp32), floorf as exact.

The ops are called at _ops level with explicit operands (the relu mask of bn_bwd / act_bwd_bias is an INPUT, nothing to excuse); where a
wrapper hides a choice (workspace or atomics, `accumulate`, a range slot of the caller) the call goes through the C ABI.
GS = (1, 132, 256, 64) is 540 672 quads, just past the 2048-block cap of shdr::stream_grid and no multiple of it; it is the LOOP DOMAIN
of a kernel: where that is the smaller side of the op the other tensor is 4x that.  Scalar kernels get NS = 540 672 + 77 elements.
Large operands are generated on the device from integers; their expectations are integer arithmetic (exact) or are checked on the
host after one copy.
"""
import ctypes

import numpy as np
import pytest
import torch

import tape_ref as F

pytestmark = pytest.mark.gpu
U = F.U32
GS = (1, 132, 256, 64)
NS = 540672 + 77
SPATIAL = [(1, 1, 1), (1, 2, 2), (1, 2, 3), (2, 5, 7), (1, 7, 9), (1, 16, 12)]
CHANNELS = [4, 12, 20, 64, 132]             # one quad; 3 quads (no power of two); 5; 16; past gap's 64-channel block
EPS = 1e-3
# assumed accuracy of the device library, in units of 2^-24 relative to the result (2 units = 1 fp32 ulp)
RSQRT = 4                                   # rsqrtf: 2 ulps (assumed, as in test_gpu_fp16_elem.py)
LOGF = 4                                    # logf: 2 ulps (assumed)
TANHF = 4                                   # tanhf: 2 ulps (assumed)
SQRTF = 1                                   # sqrtf: correctly rounded (assumed: HIP's default fp32 sqrt)
THR = float(np.float32(0.12))               # the blend threshold as the kernels receive it


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


def fd(a):
    """host array -> fp32 device tensor (int8 data is widened on the device)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.int8:
        return torch.from_numpy(a).cuda().float()
    return torch.from_numpy(a.astype(np.float32)).cuda()


def back(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape, dtype=np.int8)


def dyadic(rng, shape, lo, hi, bits=10):
    """multiples of 2^-bits in [lo, hi]"""
    return rng.integers(int(lo * 2 ** bits), int(hi * 2 ** bits) + 1, size=shape) / float(2 ** bits)


def f32(rng, shape, scale=1.0):
    return (rng.normal(size=shape) * scale).astype(np.float32)


def dev_ints(shape, lo, hi, seed):
    """integers generated on the device (large cases), as fp32"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=g, dtype=torch.int32).float()


def unaligned(t):
    """the same values at an address 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def assert_bar(got, ref, bar, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), ref.shape)
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


def observed(name, got, ref, scale=None):
    """print the worst distance to float64 in fp32 ulps of the reference (or of `scale`)"""
    ref = np.asarray(ref, dtype=np.float64)
    u = F.ulp32(ref if scale is None else scale)
    print("\nobserved %s: %.3f ulp" % (name, float((np.abs(np.asarray(got, dtype=np.float64) - ref) / u).max())))


def call(lib, K, fn, *args):
    rc = getattr(lib, fn)(*args, K._stream())
    assert rc == 0, (fn, rc, lib.shdr_last_error())


def P(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def domain(shape, sh=1, sw=1):
    n, h, w, c = shape
    return (n, h * sh, w * sw, c)


# ---- moves and selections: exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 7, 1024, NS + 2], ids=str)          # n % 4 in {0, 1, 3}: the scalar tail; NS + 2: n % 4 == 3 past the cap
def test_clip_and_clip_bwd_exact(K, n):
    rng = np.random.default_rng(n)
    x = dyadic(rng, n, -0.5, 1.5).astype(np.float32)
    x[:min(n, 4)] = np.array([0.0, 1.0, -2.0 ** -10, 1.0 + 2.0 ** -10], dtype=np.float32)[:min(n, 4)]      # exactly at lo and hi, one step outside
    x[-1] = 1.0
    dy = ints(rng, n, -8, 8)
    dy[dy == 0] = 3
    xd = fd(x)
    assert_equal(back(K.clip(xd, 0.0, 1.0)), F.clip(x, 0.0, 1.0))
    assert_equal(back(K.clip_bwd(fd(dy), xd, 0.0, 1.0)), F.clip_bwd(dy, x, 0.0, 1.0))      # closed interval: the ends pass


@pytest.mark.parametrize("npix", [1, 35, NS], ids=str)          # NS pixels: the per-pixel kernels past the cap
def test_pixel_moves_exact(K, npix):
    """pack3 / unpack3 / reverse3 / pad_channels / vgg_preprocess_bwd / alpha_blend_bwd: only moves and exact products"""
    rng = np.random.default_rng(npix)
    shape = (1, npix, 1, 3)
    srcs = [dyadic(rng, shape, -1, 1) for _ in range(4)]
    for ns, oc in ((1, 3), (1, 4), (2, 8), (3, 9), (4, 16)):
        if npix > 1000 and (ns, oc) != (3, 9):
            continue
        y = K.pack3([fd(s) for s in srcs[:ns]], oc)
        assert_equal(back(y), F.pack3(srcs[:ns], oc))
        outs = K.unpack3(y, ns)
        assert len(outs) == ns
        for o, s in zip(outs, srcs):
            assert_equal(back(o), s)
    assert_equal(back(K.reverse3(fd(srcs[0]))), F.reverse3(srcs[0]))
    for cin, cout in ((3, 4), (3, 16), (5, 8), (1, 4)):
        if npix > 1000 and cout != 4:
            continue
        x = dyadic(rng, (1, npix, 1, cin), -1, 1)
        assert_equal(back(K.pad_channels(fd(x), cout)), F.pad_channels(x, cout))
    for ic in (3, 4):
        g = ints(rng, (1, npix, 1, ic), -8, 8)
        assert_equal(back(K.vgg_preprocess_bwd(fd(g))), F.vgg_preprocess_bwd(g))           # 255 * integer: exact
    al = dyadic(rng, (1, npix, 1, 1), 0, 1, bits=7)
    dA = dyadic(rng, shape, -2, 2)
    assert_equal(back(K.alpha_blend_bwd(fd(dA), fd(al))), F.alpha_blend_bwd(dA, al))        # 2^-7 x 2^-10 multiples: exact


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 5, 7, 12), NS], ids=str)
def test_add_exact_and_range_slot(K, lib, shape):
    rng = np.random.default_rng(7)
    a, b = ints(rng, shape, -60, 60), ints(rng, shape, -60, 60)
    y = K.add(fd(a), fd(b))
    want = a.astype(np.int16) + b
    assert_equal(back(y), want)
    slot = K._range_of(y)
    assert float(back(slot)[0]) == float(np.abs(want).max())                    # the slot is max |out|, bit for bit
    # a slot that already holds a larger value is left alone
    big = torch.full((1,), 1000.0, device="cuda")
    ad, bd, yd = fd(a), fd(b), torch.empty(a.size, device="cuda")
    call(lib, K, "shdr_add_ranged_f32", P(ad), P(bd), P(yd), a.size, P(big))
    assert float(back(big)[0]) == 1000.0 and torch.equal(yd.view(y.shape), y)


# ---- pools -------------------------------------------------------------------------------------------------------------------------
def each_channel(spatial):
    return [spatial + (c,) for c in CHANNELS]


@pytest.mark.parametrize("nhw", [s for s in SPATIAL if s[1] >= 2] + ["large"], ids=str)
def test_avgpool2_exact(K, nhw):
    """integers in [-8, 8]: the four-sum and the quarter are exact.  Odd H / W: the last row / column takes no part forward and comes
    back as zero.  large: the OUTPUT (forward) and the INPUT gradient (backward) are the grid-stride domain"""
    rng = np.random.default_rng(11)
    for shape in ([domain(GS, 2, 2)] if nhw == "large" else each_channel(nhw)):
        x = ints(rng, shape, -8, 8)
        assert_equal(back(K.avgpool2(fd(x))), F.avgpool2(x))
        xs = GS if nhw == "large" else shape
        dy = ints(rng, (xs[0], xs[1] // 2, xs[2] // 2, xs[3]), -8, 8)
        dx = K.avgpool2_bwd(fd(dy), xs)
        assert tuple(dx.shape) == tuple(xs)
        assert_equal(back(dx), F.avgpool2_bwd(dy, xs))


def exactly_once(dx, dy, k):
    """disjoint k x k windows: one non-zero cell per window, and it holds the window's gradient"""
    n, ho, wo, c = dy.shape
    win = dx.reshape(n, ho, k, wo, k, c)
    assert_equal((win != 0).sum(axis=(2, 4)), np.ones(dy.shape))
    assert_equal(win.sum(axis=(2, 4)), dy)


@pytest.mark.parametrize("nhw", [(1, 2, 2), (2, 4, 6), (1, 16, 12), "large"], ids=str)
def test_maxpool2_exact(K, nhw):
    """values from {0, 1, 2}: most windows tie; the gradient goes to the first maximum in row-major order, exactly once"""
    rng = np.random.default_rng(12)
    for shape in ([domain(GS, 2, 2)] if nhw == "large" else each_channel(nhw)):
        x = ints(rng, shape, 0, 2)
        xd = fd(x)
        y = K.maxpool2(xd)
        assert_equal(back(y), F.maxpool2(x))
        dy = ints(rng, tuple(y.shape), -8, 8)
        dy[dy == 0] = 5                                            # a non-zero gradient everywhere: a wrong winner always shows
        dx = back(K.maxpool2_bwd(xd, fd(dy)))
        assert_equal(dx, F.maxpool2_bwd(x, dy))
        exactly_once(dx, dy, 2)


@pytest.mark.parametrize("nhw", SPATIAL + ["large_bwd", "large_fwd"], ids=str)
def test_maxpool3s2_exact(K, nhw):
    """MaxPool2D(3, 2, SAME) at 1 x 1, 2 x 3 and odd sizes, tied windows; overlapping windows sum their integer gradients and every
    window's gradient lands exactly once (the sums per image and channel agree).  The forward loops over the OUTPUT, the backward
    over the input"""
    rng = np.random.default_rng(13)
    for shape in ({"large_bwd": [GS], "large_fwd": [domain(GS, 2, 2)]}.get(nhw) or each_channel(nhw)):
        x = ints(rng, shape, 0, 2)
        xd = fd(x)
        y = K.maxpool3s2(xd)
        assert_equal(back(y), F.maxpool3s2(x))
        if nhw == "large_fwd":
            assert tuple(y.shape) == GS
            continue
        dy = ints(rng, tuple(y.shape), -8, 8)
        dy[dy == 0] = 5
        dx = back(K.maxpool3s2_bwd(xd, y, fd(dy)))
        assert_equal(dx, F.maxpool3s2_bwd(x, dy))
        assert_equal(dx.sum(axis=(1, 2)), dy.sum(axis=(1, 2), dtype=np.int64))


@pytest.mark.parametrize("nhw", SPATIAL + ["large"], ids=str)
def test_upsample_zero2_exact(K, nhw):
    rng = np.random.default_rng(14)
    for shape in ([GS] if nhw == "large" else each_channel(nhw)):
        n, h, w, c = shape
        dy = f32(rng, (n, (h + 1) // 2, (w + 1) // 2, c))
        got = back(K.upsample_zero2(fd(dy), shape))
        np.testing.assert_array_equal(got.view(np.uint32), F.upsample_zero2(dy, shape).astype(np.float32).view(np.uint32))


# ---- resize ------------------------------------------------------------------------------------------------------------------------
RESIZE = [((1, 1, 1), "H = W = 1: both clamps on one element; bwd weights (1 + 1)(1 + 1)... all four outputs fold onto it"),
          ((1, 1, 6), "H = 1: vertical clamp, bwd row weights 1.0 + 1.0"),
          ((1, 6, 1), "W = 1"),
          ((1, 2, 3), "H = 2: no interior row (both rows fold a border)"),
          ((1, 3, 2), "W = 2"),
          ((2, 5, 7), ""), ((1, 7, 9), ""), ((1, 16, 12), "")]
RESIZE_LARGE = [((1, 1023, 511, 4), "total = 522 753, just below gridDim * 256 = 2043 * 256 = 523 008: single tail only, ragged last block"),
                ((1, 128, 256, 64), "total = 524 288 = gridDim * 256 at the cap: `e + step < total` never holds, single tail only"),
                ((1, 129, 256, 64), "total = 528 384, just above: the first 4096 threads run the paired body, the others the tail"),
                (GS, "540 672: paired body and tail")]


@pytest.mark.parametrize("nhw", [s for s, _ in RESIZE] + [s for s, _ in RESIZE_LARGE], ids=str)
def test_resize2x_exact(K, nhw):
    """integers in [-8, 8] and the dyadic weights 0.25 / 0.75: l + (c - l) w is a multiple of 1/16 at every step -- exact"""
    rng = np.random.default_rng(15)
    for shape in ([nhw] if len(nhw) == 4 else each_channel(nhw)):
        x = ints(rng, shape, -8, 8)
        got = back(K.resize2x(fd(x)))
        assert_equal(got, F.resize2x(x))
        if shape[1] == 1 and shape[2] == 1:
            assert_equal(got, np.broadcast_to(x, (1, 2, 2, shape[3])))


@pytest.mark.parametrize("nhw", [s for s, _ in RESIZE] + [GS], ids=str)
def test_resize2x_bwd_exact_and_range_slot(K, lib, nhw):
    """integer gradients, tap weights in {1, 3, 4, 9, 12, 16} / 16: exact.  The range slot is max |dx| bit for bit"""
    rng = np.random.default_rng(16)
    for shape in ([nhw] if len(nhw) == 4 else each_channel(nhw)):
        n, h, w, c = shape
        dy = ints(rng, (n, 2 * h, 2 * w, c), -8, 8)
        dyd = fd(dy)
        dx = K.resize2x_bwd(dyd, shape)
        want = F.resize2x_bwd(dy, shape)
        assert_equal(back(dx), want)
        assert float(back(K._range_of(dx))[0]) == float(np.abs(want).max())
    big = torch.full((1,), 4096.0, device="cuda")
    out = torch.empty(shape, device="cuda")
    call(lib, K, "shdr_resize2x_bwd_ranged_f32", P(dyd), P(out), n, h, w, c, P(big))
    assert float(back(big)[0]) == 4096.0 and torch.equal(out, dx)


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (1, 1, 6, 12), (1, 2, 3, 20), (2, 5, 7, 12), (1, 16, 12, 132)], ids=str)
def test_resize2x_counted(K, shape):
    rng = np.random.default_rng(17)
    x = f32(rng, shape)
    # k = 6: two nested lerps a + (b - a) w of three operations each; |b - a| <= |a| + |b| <= 4 lerp(|a|, |b|) for w in {1/4, 3/4}
    assert_bar(back(K.resize2x(fd(x))), F.resize2x(x), F.bar32(6, 4.0 * F.abs_bound("resize2x", x)), "resize2x")
    n, h, w, c = shape
    dy = f32(rng, (n, 2 * h, 2 * w, c))
    # k = 17: up to 4 x 4 taps, each one product (the weight yw * xw is exact) and one addition onto the running sum
    assert_bar(back(K.resize2x_bwd(fd(dy), shape)), F.resize2x_bwd(dy, shape), F.bar32(17, F.abs_bound("resize2x_bwd", dy, shape)), "resize2x_bwd")


# ---- global average pool -----------------------------------------------------------------------------------------------------------
GAP_SHAPES = [(1, 1, 1), (1, 2, 2), (2, 5, 7), (1, 7, 9), (1, 16, 12), (3, 67, 1), (1, 20, 13)]      # HW = 1, 4, 35, 63, 192, 67, 260


@pytest.mark.parametrize("nhw", GAP_SHAPES, ids=str)
def test_gap_divides_once(K, nhw):
    """sums of integers are exact in fp32 in any order; the mean is ONE correctly rounded division of that sum by HW: the fp32
    quotient of the two exactly representable numbers, bit for bit (sum * (1 / HW) is 1.41 ulp off at HW = 63)"""
    rng = np.random.default_rng(18)
    for shape in each_channel(nhw):
        c = shape[-1]
        x = (ints(rng, shape, -8, 8) + ((np.arange(c) % 5) - 2).astype(np.int8)).astype(np.int8)
        hw = nhw[1] * nhw[2]
        s = x.reshape(nhw[0], hw, c).sum(axis=1, dtype=np.int64)
        y = back(K.global_avg_pool(fd(x)))
        assert y.shape == (nhw[0], c)
        assert_equal(y, s.astype(np.float32) / np.float32(hw), "gap %s" % (shape,))
        assert (np.abs(y - s / float(hw)) <= 0.5 * F.ulp32(s / float(hw))).all()


@pytest.mark.parametrize("nhw", GAP_SHAPES + [GS[:3]], ids=str)
def test_gap_bwd_divides_once(K, nhw):
    """dx = dy / HW broadcast: one correctly rounded division (dy * (1 / HW) rounds twice)"""
    rng = np.random.default_rng(19)
    for shape in ([GS] if nhw == GS[:3] else each_channel(nhw)):
        n, h, w, c = shape
        dy = f32(rng, (n, c))
        got = back(K.gap_bwd(fd(dy), shape))
        want = np.broadcast_to((dy / np.float32(h * w))[:, None, None, :], shape)
        assert_equal(got, want, "gap_bwd %s" % (shape,))
        assert_bar(got, F.gap_bwd(dy, shape), 0.5 * F.ulp32(F.gap_bwd(dy, shape)), "gap_bwd vs float64")


@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (2, 5, 7, 12), (1, 67, 1, 132), (1, 20, 13, 64)], ids=str)
def test_gap_counted(K, shape):
    rng = np.random.default_rng(20)
    n, h, w, c = shape
    x = f32(rng, shape)
    # k = ceil(HW / 64) additions per accumulator + 3 of the tail loop + 2 to join the four + 15 across the pixel lanes + the division
    assert_bar(back(K.global_avg_pool(fd(x))), F.gap(x), F.bar32(-(-h * w // 64) + 21, F.abs_bound("gap", x)), "gap")


# ---- activation backward + bias gradient -------------------------------------------------------------------------------------------
def run_bias(K, lib, npix, c, act, use_ws, seed, counted=False):
    """shdr_act_bwd_bias_f32 through the C ABI (workspace or atomics).  Integer dy in [-6, 6] with a per-channel offset, y in
    {-1, 0, 1}: relu and tanh (1 - y^2 in {0, 1}) are exact, db starts from a non-zero integer vector"""
    assert 6 * npix + 5 < 2 ** 24
    dy = dev_ints((npix, c), -4, 4, seed) + ((torch.arange(c, device="cuda") % 5) - 2).float()
    y = dev_ints((npix, c), -1, 1, seed + 1) if act else None
    start = ((torch.arange(c, device="cuda") * 7) % 11 - 5).float()
    start[start == 0] = 3.0
    db = start.clone()
    dz = torch.empty_like(dy) if act else None
    ws = K._bias_ws(c, dy.device) if use_ws else None
    call(lib, K, "shdr_act_bwd_bias_f32", P(dy), P(y), P(dz), P(db), P(ws), npix, c, act)
    if act == F.ACT_NONE:
        want = dy
    elif act == F.ACT_RELU:
        want = torch.where(y > 0, dy, torch.zeros_like(dy))
    elif act == F.ACT_TANH:
        want = dy * (1.0 - y * y)
    else:
        want = None
    if want is not None:
        if act:
            assert torch.equal(dz, want), "dz"
        assert torch.equal(db, start + want.double().sum(dim=0).float()), "db = start + sum dz"
        return
    # lrelu: 0.1f is no dyadic number.  dz: k = 2 (the fp32 rounding of the constant, the product), B = 0.1 |dy|
    dyh, yh = back(dy).astype(np.float64), back(y)
    ref = F.act_grad(dyh, yh, F.ACT_LRELU)
    assert_bar(back(dz), ref, np.where(yh > 0, 0.0, F.bar32(2, 0.1 * dyh)), "dz lrelu")
    # db: an fp32 sum of npix terms (2 roundings each) onto the start, any order
    terms = np.concatenate([back(start)[None], ref], axis=0)
    assert_bar(back(db), terms.sum(axis=0), F.sum_bar(terms, axis=0, extra=2), "db lrelu")


@pytest.mark.parametrize("act", [F.ACT_NONE, F.ACT_RELU, F.ACT_LRELU, F.ACT_TANH], ids=["none", "relu", "lrelu", "tanh"])
@pytest.mark.parametrize("q", [1, 4, 256])
def test_act_bwd_bias_small(K, lib, q, act):
    """nquads in {1, 255, 65 537, 200 001} (rounded up to whole pixels): one block; a partial block; 257 blocks capped at 256 (tail
    loop twice); 200 001 > 3 x 65 536: the four-wide body under the 256 cap, then the tail"""
    for nquads in (1, 255, 65537, 200001):
        npix = -(-nquads // q)
        for use_ws in (True, False):        # (below 2^22 quads the workspace is ignored: both end in atomics)
            run_bias(K, lib, npix, 4 * q, act, use_ws, nquads + q)


BIAS_LARGE = [(16384, 1024, F.ACT_RELU, True, "nquads = 2^22 with ws: 2048 partial rows + col_fold"),
              (16384, 1024, F.ACT_RELU, False, "nquads = 2^22 without ws: 256 cap, sixteen four-wide trips, atomics"),
              (65539, 256, F.ACT_TANH, True, "nquads = 4 194 496 with ws, Q = 64: rows hold 64 quads, four threads per quad fold in LDS"),
              (32768, 1024, F.ACT_NONE, False, "nquads = 2^23 without ws: the 384 cap"),
              (65536, 1024, F.ACT_NONE, False, "nquads = 2^24 without ws: the 512 cap (268 MB, no y / dz)")]


@pytest.mark.parametrize("case", BIAS_LARGE, ids=lambda c: "%dx%d_act%d_ws%d" % c[:4])
def test_act_bwd_bias_large(K, lib, case):
    npix, c, act, use_ws, _ = case
    run_bias(K, lib, npix, c, act, use_ws, npix)


def test_act_bwd_bias_wrapper_and_fallback(K):
    """_ops.act_bwd_bias: the fused kernel where C / 4 is a power of two, act_bwd + bias_grad elsewhere (C = 12) -- same numbers"""
    rng = np.random.default_rng(21)
    for c in (12, 16, 3):
        dy, y = ints(rng, (2, 5, 7, c), -6, 6), ints(rng, (2, 5, 7, c), -1, 1)
        dz, db = K.act_bwd_bias(fd(dy), fd(y), F.ACT_RELU)
        rz, rb = F.act_bwd_bias(dy, y, F.ACT_RELU)
        assert_equal(back(dz), rz)
        assert_equal(back(db), rb)


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------------
BN_C = [(3, "scalar kernels"), (6, "scalar kernels"), (12, "vector reduce, scalar apply (Q = 3 is no power of two)"), (64, "Q = 16"),
        (1024, "QL = 256, PL = 1"), (2048, "Q = 512: second q0 pass of bn_reduce4; bn_bwd_apply4 with unit = 2")]
BN_NPIX = [1, 2, 63, 189]
BN_LARGE = (1, 129, 128, 1024)              # 16 512 pixels > 16 x 1024: the reduction grid is capped at SHDR_BN_MAX_BLOCKS; 67 MB


def bn_operands(shape, seed, masked):
    c = shape[-1]
    off = ((torch.arange(c, device="cuda") % 3) - 1).float()
    x = dev_ints(shape, -7, 7, seed) + off
    dy = dev_ints(shape, -4, 4, seed + 1) + off
    yr = dev_ints(shape, -1, 1, seed + 2) if masked else None
    return x, dy, yr


def bn_check_stats(K, lib, x, route):
    c = x.shape[-1]
    npix = x.numel() // c
    ws = K._bn_ws(c, x.device)
    mean, var = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    mm, mv = torch.full((c,), 2.0, device="cuda"), torch.full((c,), 3.0, device="cuda")
    call(lib, K, "shdr_bn_stats_f32", P(x), P(ws), P(mean), P(var), P(mm), P(mv), npix, c, 0.99)
    x2 = x.reshape(-1, c).double()
    s1, s2 = back(x2.sum(dim=0)), back((x2 * x2).sum(dim=0))              # integers below 2^53: exact
    sums = back(ws[:2 * c]).reshape(2, c)
    assert_equal(sums[0], s1, route + ": sum x")
    assert_equal(sums[1], s2, route + ": sum x^2")
    mu = s1 / float(npix)
    v = np.maximum(s2 / float(npix) - mu * mu, 0.0)
    assert_equal(back(mean), mu.astype(np.float32), route + ": mean = (float)(sum / npix)")
    # the variance is formed in double (a contraction of the subtraction moves its last bit) and rounded once
    assert_bar(back(var), v, 0.5 * F.ulp32(v) + 2.0 ** -50 * (s2 / float(npix) + mu * mu), route + ": var")
    if npix == 1:
        assert_equal(back(var), np.zeros(c))
    unb = v * npix / (npix - 1) if npix > 1 else v                        # npix = 1: the moving variance takes v itself
    # moving = old * 0.99f + (float)new * (1 - 0.99f): the two constants, the cast, two products, one sum
    assert_bar(back(mm), 2.0 * 0.99 + mu * 0.01, F.bar32(6, 2.0 + np.abs(mu)), route + ": moving mean")
    assert_bar(back(mv), 3.0 * 0.99 + unb * 0.01, F.bar32(6, 3.0 + np.abs(unb)), route + ": moving variance")
    return mean, var


def bn_check_apply(K, x, mean, var, relu, route, slot_check=False):
    c = x.shape[-1]
    rng = np.random.default_rng(c + relu)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.3, c).astype(np.float32)
    y = K.bn_train_apply(x, mean, var, fd(gamma), fd(beta), EPS, relu)
    xh, mh, vh = back(x).astype(np.float64), back(mean).astype(np.float64), back(var).astype(np.float64)
    ref = F.bn_apply(xh, mh, vh, gamma, beta, EPS, relu)
    # k = 6 + RSQRT: x - mean, the cast of eps, var + eps, rsqrtf, the product, * gamma, + beta
    B = (np.abs(xh) + np.abs(mh)) * gamma / np.sqrt(vh + EPS) + np.abs(beta)
    got = back(y)
    assert_bar(got, ref, F.bar32(6 + RSQRT, B), route + ": bn_train_apply")
    assert float(back(K._range_of(y))[0]) == float(np.abs(got).max()), route + ": range slot of y"
    return got


def bn_check_bwd(K, lib, x, dy, yr, route):
    """integer dy, x, mask and an integer-valued `mean` operand: the double sums are exact integers -- dbeta exact, dgamma and dx
    (which carry rsqrtf) held to their bars; dgamma / dbeta are ADDED into non-zero buffers"""
    c = x.shape[-1]
    npix = x.numel() // c
    rng = np.random.default_rng(c + npix)
    mean = ((np.arange(c) % 5) - 2).astype(np.float32)
    var = rng.uniform(0.5, 30.0, c).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, c).astype(np.float32)
    g0, b0 = ((np.arange(c) % 7) - 3).astype(np.float32), ((np.arange(c) % 9) - 4).astype(np.float32)
    dgamma, dbeta = fd(g0), fd(b0)
    dx, dg, db = K.bn_bwd(dy, x, yr, fd(mean), fd(var), fd(gamma), EPS, dgamma_out=dgamma, dbeta_out=dbeta)
    assert dg is dgamma and db is dbeta
    gm = dy if yr is None else torch.where(yr > 0, dy, torch.zeros_like(dy))
    gm2, xc2 = gm.reshape(-1, c).double(), x.reshape(-1, c).double() - fd(mean).double()
    s1, s2 = back(gm2.sum(dim=0)), back((gm2 * xc2).sum(dim=0))
    a1, a2 = back(gm2.abs().sum(dim=0)), back((gm2 * xc2).abs().sum(dim=0))
    assert 6 * npix + 5 < 2 ** 24
    assert_equal(back(db), b0 + s1, route + ": dbeta = start + sum dy'")
    rstd = 1.0 / np.sqrt(var.astype(np.float64) + EPS)
    # dgamma: the cast of eps, var + eps, rsqrtf, the cast of the double product, the accumulation
    assert_bar(back(dg), g0 + s2 * rstd, F.bar32(4 + RSQRT, np.abs(s2) * rstd + np.abs(g0)), route + ": dgamma")
    # dx = ga (g - m1 - xh m2): invstd 2 + RSQRT = 6; ga = gamma invstd 7; m1 a cast 1; m2 = (float)(S2 / n) invstd 8; xh = (x - mu) invstd 8;
    # xh m2 17; the two subtractions 19; the product 27.  B = |ga| (|g| + mean |dy'| + |xh| mean(|dy' (x - mean)|) rstd)
    k0 = gamma.astype(np.float64) * rstd
    g, xc = back(gm2), back(xc2)
    ref = k0 * (g - s1 / float(npix) - xc * rstd * (s2 / float(npix)) * rstd)
    B = k0 * (np.abs(g) + a1 / float(npix) + np.abs(xc) * rstd * (a2 / float(npix)) * rstd)
    got = back(dx).reshape(-1, c).astype(np.float64)
    assert_bar(got, ref, F.bar32(23 + RSQRT, B), route + ": dx")
    assert float(back(K._range_of(dx))[0]) == float(np.abs(got).max()), route + ": range slot of dx"
    return got, back(dg), back(db)


@pytest.mark.parametrize("c", [c for c, _ in BN_C])
def test_batchnorm_small(K, lib, c, monkeypatch):
    """bn_stats, bn_train_apply, bn_bwd with and without the relu mask at npix in {1, 2, 63, 189}; then the same operands through the
    scalar kernels (SHDR_BN_SCALAR) and through the unaligned fallback (views offset by one float): the same numbers"""
    for npix in BN_NPIX:
        shape = (1, 1, npix, c)
        results = {}
        for route in ("default", "unaligned", "scalar"):
            if route == "scalar":
                monkeypatch.setenv("SHDR_BN_SCALAR", "1")
            x, dy, yr = bn_operands(shape, c + npix, True)
            if route == "unaligned":
                x, dy, yr = unaligned(x), unaligned(dy), unaligned(yr)
            mean, var = bn_check_stats(K, lib, x, route)
            out = [back(mean), back(var)]
            for relu in (False, True):
                out.append(bn_check_apply(K, x, mean, var, relu, route))
            for mask in (None, yr):
                out.extend(bn_check_bwd(K, lib, x, dy, mask, route))
            results[route] = out
        monkeypatch.delenv("SHDR_BN_SCALAR")
        # [mean, var, y, y_relu, (dx, dgamma, dbeta) x 2]: the sums are exact in double, so every result has the same bits on every route
        # -- except dx where the default route took bn_bwd_apply4 (C % 4 == 0 and C / 4 a power of two: C = 64, 1024, 2048) and the
        # fallbacks bn_bwd_apply: two kernels whose expressions the compiler may contract differently; each is held to its bar above.
        # At C = 3, 6 and 12 (Q = 3) every route runs bn_bwd_apply: the same bits
        q = c // 4
        took_apply4 = c % 4 == 0 and q & (q - 1) == 0
        for route in ("unaligned", "scalar"):
            for i, (a, b) in enumerate(zip(results["default"], results[route])):
                if i not in (4, 7) or not took_apply4:
                    assert_equal(a, b, "%s, result %d" % (route, i))


def test_batchnorm_large(K, lib):
    """16 512 pixels x 1024 channels: the block cap of bn_reduce4 (SHDR_BN_MAX_BLOCKS), four-wide body + tail; apply kernels past 2048 blocks"""
    x, dy, yr = bn_operands(BN_LARGE, 5, True)
    mean, var = bn_check_stats(K, lib, x, "large")
    bn_check_apply(K, x, mean, var, True, "large")
    bn_check_bwd(K, lib, x, dy, yr, "large")


def test_range_slot_prefilled_is_left_alone(K, lib):
    """bn_train_apply / bn_bwd with a slot that already holds a larger value"""
    x, dy, yr = bn_operands((1, 5, 7, 64), 9, True)
    c = 64
    one, big = torch.ones(c, device="cuda"), torch.full((1,), 1.0e6, device="cuda")
    y = torch.empty_like(x)
    call(lib, K, "shdr_bn_train_apply_ranged_f32", P(x), P(one), P(one), P(one), P(one), P(y), 35, c, EPS, 0, P(big))
    ws, dg, db, dx = K._bn_ws(c, x.device), torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.empty_like(x)
    call(lib, K, "shdr_bn_bwd_ranged_f32", P(dy), P(x), P(yr), P(one), P(one), P(one), P(ws), P(dg), P(db), P(dx), 35, c, EPS, P(big))
    assert float(back(big)[0]) == 1.0e6 and float(back(y).max()) > 1.0


# ---- affine_act --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [F.ACT_NONE, F.ACT_RELU, F.ACT_LRELU, F.ACT_TANH], ids=["none", "relu", "lrelu", "tanh"])
@pytest.mark.parametrize("c,route", [(3, "scalar"), (12, "vector"), (12, "unaligned"), (64, "large")])
def test_affine_act(K, c, route, a):
    """the 2^3 presence combinations of scale / shift / residual; C = 3: the scalar kernel, C = 12: float4; a view offset by one float:
    the scalar kernel on the same numbers; large: past the cap"""
    rng = np.random.default_rng(c + a)
    shape = GS if route == "large" else (2, 5, 7, c)
    xi, ri = ints(rng, shape, -8, 8), ints(rng, shape, -8, 8)
    si, ti = ints(rng, c, -3, 3), ints(rng, c, -8, 8)
    x, r, s, t = f32(rng, shape), f32(rng, shape), f32(rng, c), f32(rng, c)
    for use in range(8):
        if route == "large" and use != 7:
            continue
        pick = lambda sc, sh, re: (sc if use & 1 else None, sh if use & 2 else None, re if use & 4 else None)
        dev = lambda v: None if v is None else (unaligned(fd(v)) if route == "unaligned" else fd(v))
        if a in (F.ACT_NONE, F.ACT_RELU):                            # integers: exact
            sc, sh, re = pick(si, ti, ri)
            got = back(K.affine_act(dev(xi), dev(sc), dev(sh), dev(re), a))
            assert_equal(got, F.affine_act(xi, sc, sh, re, a), "affine_act exact %d" % use)
        sc, sh, re = pick(s, t, r)
        got = back(K.affine_act(dev(x), dev(sc), dev(sh), dev(re), a))
        pre, ref = F.affine_pre(x, sc, sh, re), F.affine_act(x, sc, sh, re, a)
        # up to three roundings before the activation (|act'| <= 1 carries them through), B = |x| |scale| + |shift| + |residual|;
        # lrelu: the constant and the product; tanh: the assumed TANHF
        bar = F.bar32(3, F.affine_pre(x, sc, sh, re, absolute=True)) + F.bar32({F.ACT_LRELU: 2, F.ACT_TANH: TANHF}.get(a, 0), ref)
        assert_bar(got, ref, bar, "affine_act %d" % use)
        if a == F.ACT_TANH and use == 0:
            observed("tanhf (affine_act, |x| < 5)", got, np.tanh(pre))


# ---- inverse-CRF head ----------------------------------------------------------------------------------------------------------------
def knot_x(K_, rng, n):
    """fp32 x with fp32(K - 1) * x an exact integer k (a table knot), found on the host"""
    k = rng.integers(0, K_, size=4 * n + 8)
    x = (k / np.float32(K_ - 1)).astype(np.float32)
    ok = (np.float32(K_ - 1) * x).astype(np.float32) == k
    assert ok.sum() >= n
    return x[ok][:n], k[ok][:n]


@pytest.mark.parametrize("K_", [2, 1024, 8192])
@pytest.mark.parametrize("npb", [1, 3, 4, 5, 1027, 1048884, 1048885], ids=str)
def test_apply_rf_counted(K, K_, npb):
    """n_per_batch & 3 == 0: the float4 loop (1 048 884 = 4 x (1024 x 256 + 77): past its 1024-block cap); else the scalar loop
    (1 048 885: past the cap).  x holds 0, 1, exact knots, values just below a knot and uniform ones"""
    rng = np.random.default_rng(K_ + npb)
    nb = 2 if npb < 10 ** 6 else 1
    x = rng.random((nb, npb)).astype(np.float32)
    kx, kk = knot_x(K_, rng, min(npb, 64))
    spec = np.concatenate([[0.0, 1.0], kx, np.nextafter(kx[kk > 0], np.float32(0))]).astype(np.float32)
    m = min(npb, spec.size)
    x[0, :m] = rng.permutation(spec)[:m]
    rf = np.sort(rng.random((nb, K_)), axis=1).astype(np.float32)
    got = back(K.apply_rf(fd(x), fd(rf)))
    yv, i0, i1, w0, w1 = F.apply_rf_parts(x, K_)
    l0, l1 = np.take_along_axis(rf.astype(np.float64), i0, 1), np.take_along_axis(rf.astype(np.float64), i1, 1)
    # yv = (K - 1) x rounds once: it moves the result by at most 2^-24 yv times the steepest adjacent table step (the function is
    # continuous across a knot, so a floor taken on the other side changes nothing more); y1 - yv and yv - y0 are exact; two products
    # and the sum: k = 3 on |l0| + |l1|
    step = np.abs(np.diff(rf.astype(np.float64), axis=1))
    sp = np.pad(step, ((0, 0), (1, 1)), mode="edge")
    D = np.maximum(np.maximum(np.take_along_axis(sp, i0, 1), np.take_along_axis(sp, i0 + 1, 1)), np.take_along_axis(sp, np.minimum(i0 + 2, K_), 1))
    assert_bar(got, F.apply_rf(x, rf), U * yv * D + F.bar32(3, np.abs(l0) + np.abs(l1)), "apply_rf")
    on = np.isin(x, kx) | (x == 0) | (x == 1)
    assert_equal(got[on], np.take_along_axis(rf, np.rint(yv).astype(np.int64), 1)[on], "on a knot: the table entry itself")


@pytest.mark.parametrize("K_", [2, 1024, 8192])
# the issue's {1, 3, 4, 5, 1027} (the backward has no `& 3` branch: one scalar loop); 70 001 > 256 blocks x 256: past the cap of apply_rf_bwd
@pytest.mark.parametrize("npb", [1, 3, 4, 5, 1027, 70001], ids=str)
def test_apply_rf_bwd(K, K_, npb):
    rng = np.random.default_rng(K_ * 3 + npb)
    nb = 2
    rf = np.sort(rng.random((nb, K_)), axis=1).astype(np.float32)
    # (1) x on exact knots, integer dy: every weight is 1 or 0, drf[k] is the integer sum of the gradients that hit knot k -- exact
    kx, kk = knot_x(K_, rng, nb * npb)
    x, dy = kx.reshape(nb, npb), ints(rng, (nb, npb), -8, 8)
    want = np.zeros((nb, K_))
    np.add.at(want, (np.repeat(np.arange(nb), npb), kk), dy.reshape(-1))
    for need_dx in (False, True):
        drf, dx = K.apply_rf_bwd(fd(x), fd(rf), fd(dy), need_dx)
        assert (dx is not None) == need_dx
        assert_equal(back(drf), want, "drf on knots, need_dx=%d" % need_dx)
    # (2) x strictly inside the intervals (the floor is the same in fp32 and fp64), random dy
    k0 = rng.integers(0, K_ - 1, size=(nb, npb))
    x = ((k0 + rng.uniform(0.05, 0.95, size=(nb, npb))) / (K_ - 1)).astype(np.float32)
    dy = f32(rng, (nb, npb))
    drf, dx = K.apply_rf_bwd(fd(x), fd(rf), fd(dy), True)
    rdrf, rdx = F.apply_rf_bwd(x, rf, dy)
    _, adx = F.apply_rf_bwd(x, rf, dy, absolute=True)
    # dx = g km1 (l1 - l0): two products and the difference, k = 3, B = |g| (K - 1) (|l0| + |l1|)
    assert_bar(back(dx), rdx, F.bar32(3, adx), "dx")
    # drf[k]: each term g w carries the rounding of yv (absolute 2^-24 yv on w) and of the product; the n_k terms of a bin meet in LDS
    # and global atomics in any order, onto zero: (n_k + 1) 2^-24 sum |terms|
    yv, i0, i1, w0, w1 = F.apply_rf_parts(x, K_)
    g = np.abs(dy.astype(np.float64))
    acc, cnt = np.zeros((nb, K_)), np.zeros((nb, K_))
    rows = np.broadcast_to(np.arange(nb)[:, None], i0.shape)
    for idx, wt in ((i0, w0), (i1, w1)):
        np.add.at(acc, (rows, idx), g * (yv + wt))
        np.add.at(cnt, (rows, idx), 1.0)
    adrf, _ = F.apply_rf_bwd(x, rf, dy, absolute=True)
    assert_bar(back(drf), rdrf, U * acc + (cnt + 1) * U * adrf, "drf")


def increase_rows(rng, k):
    """fp32 rows: monotone; one negative step in the middle; the minimum at the first gap; at the last gap.  Ties in the minimum are
    excluded (every other gap is >= 0.05, the negative one is unique): the kernel documents first-minimum, TF spreads the gradient"""
    rows = []
    for kind in range(4):
        g = rng.random(k - 1) + 0.05
        if kind and k > 2:
            g[{1: (k - 1) // 2, 2: 0, 3: k - 2}[kind]] = -0.5
        rows.append(np.concatenate([[0.0], np.cumsum(g)]))
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("K_", [2, 3, 257, 1024, 4096])
def test_increase_and_bwd_counted(K, K_):
    rng = np.random.default_rng(K_)
    rf = increase_rows(rng, K_)
    G = K_ - 1
    got = back(K.increase(fd(rf)))
    ref = F.increase(rf)
    # a gap: the difference and + r, 2; their sum S: ceil(G / 256) per thread + 6 in the wave + 2 across; g / S: 1; the running sum of
    # out[k]: k - 1.  Every term is >= 0, so the bound is relative to the result
    kS = -(-G // 256) + 8
    assert_bar(got, ref, F.bar32(kS + 3 + np.arange(K_)[None, :], ref), "increase")
    assert_equal(got[:, 0], np.zeros(4))
    assert (np.diff(got.astype(np.float64), axis=1) >= 0).all()      # non-decreasing bit for bit (the reason for the sequential scan)
    dout = f32(rng, rf.shape)
    got = back(K.increase_bwd(fd(rf), fd(dout)))
    ref = F.increase_bwd(rf, dout)
    # d[k] = dn[k] / S - D / S^2: dn a sequential sum of up to G terms; S as above (+ 2 per term), twice in S^2; D a block sum of products.
    # kd = G + 3 (kS + 2) + kS + 6 on Bd = sum_{j>=k} |dout| / S + sum |dn| ng / S^2.  The argmin term subtracts the block sum of all d;
    # drf[k] = d[k-1] - d[k]
    g = rf.astype(np.float64)[:, 1:] - rf.astype(np.float64)[:, :-1]
    mn = g.min(axis=1, keepdims=True)
    ng = g + np.maximum(-mn, 0.0)
    S = ng.sum(axis=1, keepdims=True)
    dna = np.cumsum(np.abs(dout.astype(np.float64))[:, :0:-1], axis=1)[:, ::-1]
    Bd = dna / S + (dna * ng).sum(axis=1, keepdims=True) / (S * S)
    kd = G + 4 * kS + 12
    bd = F.bar32(kd, Bd)
    neg = (mn < 0)[:, 0]
    bd[neg, g.argmin(axis=1)[neg]] += F.bar32(kd + kS, Bd.sum(axis=1))[neg]
    bar = np.zeros(rf.shape)
    bar[:, 1:] += bd
    bar[:, :-1] += bd
    Bout = np.zeros(rf.shape)
    Bout[:, 1:] += Bd
    Bout[:, :-1] += Bd
    assert_bar(got, ref, bar + F.bar32(1, Bout), "increase_bwd")


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("f", [1, 255, 512])
def test_invcrf_decode_and_bwd_exact(K, b, f):
    """integer table rows, weights, features and gradients: every dot product is an exact integer (K = 1024)"""
    rng = np.random.default_rng(b * 7 + f)
    k = 1024
    table, wfc, bfc, feat = ints(rng, (k, 12), -3, 3), ints(rng, (f, 11), -2, 2), ints(rng, 11, -4, 4), ints(rng, (b, f), -3, 3)
    assert_equal(back(K.invcrf_decode(fd(feat), fd(wfc), fd(bfc), fd(table))), F.invcrf_decode(feat, wfc, bfc, table))
    dinv = ints(rng, (b, k), -3, 3)
    dfeat, dwfc, dbfc = K.invcrf_decode_bwd(fd(dinv), fd(feat), fd(wfc), fd(table))
    rf_, rw, rb = F.invcrf_decode_bwd(dinv, feat, wfc, table)
    assert np.abs(rw).max() < 2 ** 24
    assert_equal(back(dfeat), rf_)
    assert_equal(back(dwfc), rw)
    assert_equal(back(dbfc), rb)


# ---- losses --------------------------------------------------------------------------------------------------------------------------
NPER = [1, 255, 257, 33000]                 # 33 000 > 128 blocks x 256: past the cap of diff_loss / sample_dot
PER_SAMPLE = [(nb, n) for nb in (1, 3) for n in NPER] + [(1, NS)]      # the elementwise kernels: one case past 2048 blocks


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("npb", NPER)
def test_diff_loss_and_sample_dot(K, nb, npb):
    """a - b a multiple of 1/4 in [-2, 2]: squares, absolute values and all their partial sums are exact.  sample_dot: exact.
    diff_loss: every block divides ITS partial sum by n and the blocks meet in atomics: k = blocks roundings on the (non-negative)
    result; with one block that is the correctly rounded quotient"""
    rng = np.random.default_rng(nb + npb)
    a, b = dyadic(rng, (nb, npb, 1, 1), -1, 1, bits=2), dyadic(rng, (nb, npb, 1, 1), -1, 1, bits=2)
    blocks = min(-(-npb // 256), 128)
    for mode in (0, 1):
        ref = F.diff_loss(a, b, mode)
        assert_bar(back(K.diff_loss(fd(a), fd(b), mode)), ref, F.bar32(blocks, ref), "diff_loss mode %d" % mode)
    ai, bi = ints(rng, (nb, npb), -4, 4), ints(rng, (nb, npb), -4, 4)
    assert_equal(back(K.sample_dot(fd(ai))), F.sample_dot(ai))
    assert_equal(back(K.sample_dot(fd(ai), fd(bi))), F.sample_dot(ai, bi))


@pytest.mark.parametrize("nb,npb", PER_SAMPLE)
def test_diff_loss_bwd_counted(K, lib, nb, npb):
    """gb = g[b] / n ONE rounding (the reference divides once); mode 1: +-gb, k = 1; mode 0: (2 d) gb, d exact here, k = 2;
    accumulate: + 1 on |da0| + |v|"""
    rng = np.random.default_rng(nb * 5 + npb)
    a, b = dyadic(rng, (nb, npb), -1, 1), dyadic(rng, (nb, npb), -1, 1)
    g, da0 = f32(rng, nb), f32(rng, (nb, npb))
    ad, bd, gd = fd(a), fd(b), fd(g)
    for mode in (0, 1):
        ref = F.diff_loss_bwd(a, b, g, mode)
        got = back(K.diff_loss_bwd(ad, bd, gd, mode))
        assert_bar(got, ref, F.bar32(2 - mode, ref), "diff_loss_bwd mode %d" % mode)
        if mode:                  # +-(g / n): the correctly rounded fp32 quotient, bit for bit (g * (1 / n) is not)
            assert_equal(got, np.sign(a - b) * (g / np.float32(npb))[:, None], "diff_loss_bwd mode 1 divides once")
        for acc in (0, 1):
            da = fd(da0)
            call(lib, K, "shdr_diff_loss_bwd_f32", P(ad), P(bd), P(gd), P(da), nb, npb, mode, acc)
            want = F.diff_loss_bwd(a, b, g, mode, da0 if acc else None)
            assert_bar(back(da), want, F.bar32(2 - mode, ref) + acc * F.bar32(1, np.abs(da0) + np.abs(ref)), "accumulate=%d mode %d" % (acc, mode))


TV_SHAPES = [(1, 1, 1, 3), (1, 1, 6, 3), (2, 6, 1, 3), (2, 5, 7, 3), (1, 16, 12, 4), (1, 211, 277, 3), (1, 419, 431, 3)]
# (1, 211, 277, 3): 175 341 elements, 685 blocks > the 512 cap of tv_loss; (1, 419, 431, 3): 541 767 > 2048 x 256 for tv_loss_bwd


@pytest.mark.parametrize("shape", TV_SHAPES, ids=str)
def test_tv_loss_and_bwd(K, lib, shape):
    """integer y: the differences and their partial sums are exact; every block divides its partial sum by the element count:
    k = blocks.  Backward: gs = g / total (1), gs * d with d an integer in [-4, 4] (1), accumulate + 1"""
    rng = np.random.default_rng(sum(shape))
    y = ints(rng, shape, -8, 8)
    yd = fd(y)
    ref = F.tv_loss(y)
    blocks = min(-(-y.size // 256), 512)
    got = back(K.tv_loss(yd))
    assert got.shape == (1,)
    assert_bar(got, [ref], F.bar32(blocks, ref), "tv_loss")
    g, dy0 = np.float32([0.7]), f32(rng, shape)
    gd = fd(g)
    want = F.tv_loss_bwd(y, g)
    assert_bar(back(K.tv_loss_bwd(yd, gd)), want, F.bar32(2, want), "tv_loss_bwd")
    for acc in (0, 1):
        d = fd(dy0)
        call(lib, K, "shdr_tv_loss_bwd_f32", P(yd), P(gd), P(d), *shape, acc)
        assert_bar(back(d), F.tv_loss_bwd(y, g, dy0 if acc else None), F.bar32(2, want) + acc * F.bar32(1, np.abs(dy0) + np.abs(want)),
                   "tv_loss_bwd accumulate=%d" % acc)


@pytest.mark.parametrize("nb,npb", PER_SAMPLE)
def test_mean_norm(K, nb, npb):
    rng = np.random.default_rng(nb + npb * 3)
    r = (np.abs(f32(rng, (nb, npb, 1, 1))) + np.float32(0.1)).astype(np.float32)
    g = f32(rng, r.shape)
    rd, gd = fd(r), fd(g)
    ssum, gdot = K.sample_dot(rd), K.sample_dot(gd, rd)
    sh, gh = back(ssum).astype(np.float64), back(gdot).astype(np.float64)      # the sums the kernels are given (checked above)
    eps, target = float(np.float32(1e-6)), 0.5
    # forward: m = sum / n, eps + m, r / (.), * target: k = 4 (the reference divides once)
    ref = F.mean_norm_fwd(r, sh, eps, target)
    assert_bar(back(K.mean_norm_fwd(rd, ssum, eps, target)), ref, F.bar32(4, ref), "mean_norm_fwd")
    # mean_norm sums r itself (sample_dot, atomics in any order): against the exact sum, with the depth of that sum of positive terms --
    # ceil(n / (blocks x 256)) per thread + 6 in the wave + 2 across + the atomics of the blocks
    blocks = min(-(-npb // 256), 128)
    depth = -(-npb // (blocks * 256)) + 8 + blocks
    ref = F.mean_norm_fwd(r, F.sample_dot(r), eps, target)
    assert_bar(back(K.mean_norm(rd, eps, target)), ref, F.bar32(4 + depth, ref), "mean_norm")
    # backward: d 2; g / d 3; n d d 2 + 2 + 2, the quotient 7; the difference 8; * target 9
    assert_bar(back(K.mean_norm_bwd(gd, ssum, gdot, eps, target)), F.mean_norm_bwd(g, sh, gh, eps, target),
               F.bar32(9, F.mean_norm_bwd(g, sh, gh, eps, target, absolute=True)), "mean_norm_bwd")


# ---- logc, alpha, vgg ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, NS])
def test_logc_and_bwd_counted(K, n):
    rng = np.random.default_rng(n)
    x = (rng.random(n) * 4.0).astype(np.float32)
    x[0] = 0.0
    got = back(K.logc(fd(x)))
    ref = F.logc(x)
    # the argument 1 + 10 x: 2 roundings, which move the logarithm by at most 2 x 2^-24 in ABSOLUTE terms (d log a = da / a); logf;
    # inv = 1 / logf(11): LOGF + 1; the product 1 -- relative to the result
    assert_bar(got, ref, 2 * U / np.log(11.0) + F.bar32(2 * LOGF + 2, ref), "logc")
    dy = f32(rng, n)
    ref = F.logc_bwd(dy, x)
    # k = 10 / logf(11): LOGF + 1; dy k 1; 10 x, 1 + .: 2; the division 1
    assert_bar(back(K.logc_bwd(fd(dy), fd(x))), ref, F.bar32(LOGF + 5, ref), "logc_bwd")


@pytest.mark.parametrize("npix", [1, 35, NS])
def test_alpha_mask_and_blend(K, npix):
    rng = np.random.default_rng(npix)
    shape = (1, npix, 1, 3)
    # (1) thr = 1/8 and dyadic operands: every step is exact.  The maximum sits exactly at 1 - thr (alpha 0), at 1 (alpha 1), in between
    b = dyadic(rng, shape, 0.5, 1.25)
    b.reshape(-1, 3)[:min(npix, 3), 0] = np.array([0.875, 1.0, 2.0])[:min(npix, 3)]
    b.reshape(-1, 3)[:min(npix, 3), 1:] = 0.5
    hal, dA = dyadic(rng, shape, -2, 2, bits=6), dyadic(rng, shape, -2, 2, bits=6)
    ra, ral = F.alpha_blend(b, hal, 0.125)
    assert_equal(back(K.alpha_mask(fd(b), 0.125)), ral)
    assert ral.reshape(-1)[:min(npix, 3)].tolist() == [0.0, 1.0, 1.0][:min(npix, 3)]
    a, al = K.alpha_blend(fd(b), fd(hal), 0.125, return_alpha=True)
    assert_equal(back(a), ra)
    assert_equal(back(al), ral)
    assert_equal(back(K.alpha_blend(fd(b), fd(hal), 0.125)), ra)
    dB, dhal = K.alpha_blend_full_bwd(fd(b), fd(hal), fd(dA), 0.125)
    rB, rhal = F.alpha_blend_full_bwd(b, hal, dA, 0.125)
    assert_equal(back(dB), rB)
    assert_equal(back(dhal), rhal)
    # (2) thr = 0.12f, random operands: mx - 1, + thr, / thr: k = 3 on (|mx - 1| + thr) / thr; the blend adds a product and a sum
    b, hal = (rng.random(shape) * 0.4 + 0.75).astype(np.float32), f32(rng, shape)
    b.reshape(-1, 3)[0] = (np.float32(1) - np.float32(THR), 0.5, 0.5)
    if npix > 1:
        b.reshape(-1, 3)[1] = (0.5, 1.0, 0.5)
    ra, ral = F.alpha_blend(b, hal, THR)
    mx = b.astype(np.float64).max(axis=-1, keepdims=True)
    bal = F.bar32(3, (np.abs(mx - 1.0) + THR) / THR)
    a, al = K.alpha_blend(fd(b), fd(hal), THR, return_alpha=True)
    assert_bar(back(al), ral, bal, "alpha")
    assert_bar(back(K.alpha_mask(fd(b), THR)), ral, bal, "alpha_mask")
    if npix > 1:
        assert float(back(al).reshape(-1)[1]) == 1.0               # the maximum exactly at 1: alpha is 1, not 1 - ulp
    hr = np.abs(hal.astype(np.float64))[..., ::-1]
    assert_bar(back(a), ra, bal * hr + F.bar32(2, np.abs(b) + ral * hr), "alpha_blend")


@pytest.mark.parametrize("oc", [3, 4])
@pytest.mark.parametrize("npix", [1, 35, NS])
def test_vgg_preprocess_counted(K, npix, oc):
    rng = np.random.default_rng(npix + oc)
    x = (rng.random((1, npix, 1, 3)) * 1.25).astype(np.float32)
    got = back(K.vgg_preprocess(fd(x), oc))
    # k = 3: x * 255, the fp32 rounding of the mean constant, the subtraction; B = |x| 255 + mean
    B = F.pad_channels(np.abs(x.astype(np.float64))[..., ::-1] * 255.0 + np.asarray(F.ops.VGG_MEAN), oc)
    assert_bar(got, F.vgg_preprocess(x, oc), F.bar32(3, B), "vgg_preprocess")
    assert oc == 3 or not got[..., 3].any()


def test_device_library_calls_observed(K):
    """rsqrtf, logf and tanhf on arguments that reach them without a rounding of our own, against float64: the observed distance is
    printed (DESIGN.md 4.2 records it) and must stay inside the ASSUMED bound"""
    rng = np.random.default_rng(99)
    c = 4096
    # bn_train_apply with x - mean = 1, gamma = 1, beta = 0: y = rsqrtf(var + eps) itself; var + eps is one fp32 addition, redone here
    var = (10.0 ** rng.uniform(-4, 2, c)).astype(np.float32)
    one, zero = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    y = back(K.bn_train_apply(torch.ones(1, 1, 1, c, device="cuda"), zero, fd(var), one, zero, EPS, False)).reshape(-1)
    ref = 1.0 / np.sqrt((var + np.float32(EPS)).astype(np.float64))
    observed("rsqrtf (1e-3 <= a <= 100)", y, ref)
    assert_bar(y, ref, F.bar32(RSQRT, ref), "rsqrtf")
    # affine_act without operands: tanhf(x)
    x = (rng.normal(size=65536) * 2.0).astype(np.float32)
    y = back(K.affine_act(fd(x.reshape(1, 1, -1, 4)), act=F.ACT_TANH)).reshape(-1)
    observed("tanhf (|x| < 9)", y, np.tanh(x.astype(np.float64)))
    assert_bar(y, np.tanh(x.astype(np.float64)), F.bar32(TANHF, np.tanh(x.astype(np.float64))), "tanhf")
    # logc on multiples of 2^-6: 10 x and 1 + 10 x are exact, so the result is logf(a) * (1 / logf(11)): two logf, a division, a product
    x = (rng.integers(1, 257, size=65536) / 64.0).astype(np.float32)
    y = back(K.logc(fd(x)))
    # (logf cannot be reached alone: every kernel that calls it multiplies by 1 / logf(11) or 10 / logf(11) -- it is bounded JOINTLY)
    observed("logc on exact arguments, 1 < a <= 41 (logf twice + a division + a product: 5 ulp allowed)", y, F.logc(x))
    assert_bar(y, F.logc(x), F.bar32(2 * LOGF + 2, F.logc(x)), "logf")
    # adam_step with beta1 = beta2 = 1, lr_t = 1, eps = 0, p = 0, m = 1: m and v stay as they are and p = -(1 / sqrtf(v)) -- sqrtf and one
    # division, nothing else.  If both are correctly rounded the result is NumPy's fp32 1 / sqrt(v) bit for bit
    v = (10.0 ** rng.uniform(-12, 4, 65536)).astype(np.float32)
    pd, md, vd = torch.zeros(v.size, device="cuda"), torch.ones(v.size, device="cuda"), fd(v)
    K.adam_step(pd, torch.zeros(v.size, device="cuda"), md, vd, 1.0, 1.0, 1.0, 0.0, 1.0)
    assert_equal(back(md), np.ones(v.size))
    assert_equal(back(vd), v)
    ref = -1.0 / np.sqrt(v.astype(np.float64))
    same = back(pd) == -(np.float32(1) / np.sqrt(v))
    observed("sqrtf + one division (1e-12 <= v <= 1e4; %.4f%% equal the correctly rounded pair)" % (100.0 * same.mean()), back(pd), ref)
    assert_bar(back(pd), ref, F.bar32(SQRTF + 1, ref), "sqrtf")


# ---- soft histogram / front end backward ---------------------------------------------------------------------------------------------
# (1, 419, 418): 525 426 ELEMENTS, past the cap of soft_hist_bwd (one thread per element), ragged W.  lin_frontend_bwd runs one thread per
# PIXEL: its case past the cap is FRONT_LARGE, 527 075 pixels (2059 blocks of work on 2048), dF 202 MB
FRONT_SHAPES = [(1, 2, 2), (1, 2, 3), (2, 5, 7), (1, 7, 9), (1, 16, 12), (1, 419, 418)]
FRONT_LARGE = (1, 725, 727)


def front_image(rng, nhw):
    """multiples of 2^-10 in [0, 1]; every bin centre, bin edge and 0 / 1 occur"""
    a = rng.integers(0, 1025, size=nhw + (3,)) / 1024.0
    m = min(a.size, 33)
    a.reshape(-1)[:m] = rng.permutation(33)[:m] / 32.0
    return a.astype(np.float32)


@pytest.mark.parametrize("nhw", FRONT_SHAPES, ids=str)
def test_soft_hist_bwd_exact(K, nhw):
    """B a power of two, x a multiple of 2^-10, integer gradients: the support test and the slope -+B are exact, the sum is an integer"""
    rng = np.random.default_rng(nhw[1] * 3 + nhw[2])
    img = front_image(rng, nhw)
    for B in ((16,) if nhw[1] > 100 else (4, 8, 16, 32)):
        dy = ints(rng, nhw + (3 * B,), -8, 8)
        assert_equal(back(K.soft_hist_bwd(fd(img), fd(dy), B)), F.soft_hist_bwd(img, dy, B), "B = %d" % B)


@pytest.mark.parametrize("nhw", FRONT_SHAPES + [FRONT_LARGE], ids=str)
def test_lin_frontend_bwd(K, nhw):
    rng = np.random.default_rng(nhw[1] * 11 + nhw[2])
    img = front_image(rng, nhw)
    imgd = fd(img)
    if nhw == FRONT_LARGE:                # the second trip of the per-pixel loop (p += gridDim.x * 256, ibase of the later pixels)
        assert nhw[1] * nhw[2] > 2048 * 256 and (nhw[1] * nhw[2]) % (2048 * 256)
        dFd = dev_ints(nhw + (96,), -8, 8, 5)
        dF = back(dFd.to(torch.int8))
        return assert_equal(back(K.lin_frontend_bwd(imgd, dFd)), F.lin_frontend_bwd(img, dF), "past the cap, integer gradients: exact")
    dF = ints(rng, nhw + (96,), -8, 8)
    assert_equal(back(K.lin_frontend_bwd(imgd, fd(dF))), F.lin_frontend_bwd(img, dF), "integer gradients, integer weights: exact in any order")
    if nhw[1] > 100:
        return
    assert_equal(back(K.lin_frontend_bwd(imgd, fd(dF[..., :93].copy()))), F.lin_frontend_bwd(img, dF), "93 channels")
    dF = f32(rng, nhw + (96,))
    # the local terms: up to 6 live bins, each a product (+-B g is exact) and an addition; then the atomics of the 3 x 3 REFLECT stencil, up
    # to 36 per element at a corner of a 2 x 2 image, in any order: 6 + 36 + 1 roundings on the sum of magnitudes
    assert_bar(back(K.lin_frontend_bwd(imgd, fd(dF))), F.lin_frontend_bwd(img, dF), F.bar32(43, F.lin_frontend_bwd(img, dF, absolute=True)),
               "lin_frontend_bwd")


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1.0, 2.0 ** -7], ids=["gs1", "gs2^-7"])
@pytest.mark.parametrize("n", [1, 255, NS])
def test_adam_two_steps_counted(K, n, gs):
    """two consecutive steps against the float64 Keras formula, each from the state the device holds.
    g' = g gs 1; m: two products and the sum 3 on |b1 m| + |(1 - b1) g'| (1 - b1 is exact for 0.9f, 0.999f); v: g' g', * (1 - b2), b2 v,
    the sum: 5 + 2 for g', all terms >= 0; the update u = lr m / (sqrt(v) + eps): the root halves v's 7 and adds SQRTF, + eps 1, lr m 1, the
    division 1: 7 + SQRTF relative to |u|, plus m's absolute error scaled by lr / den; p - u: 1 on |p| + |u|"""
    rng = np.random.default_rng(n)
    b1, b2, eps = (float(np.float32(v)) for v in (0.9, 0.999, 1e-7))
    p, m, v = f32(rng, n), f32(rng, n, 0.1), (f32(rng, n, 0.1) ** 2).astype(np.float32)
    pd, md, vd = fd(p), fd(m), fd(v)
    worst = 0.0
    for step in (1, 2):
        g = (f32(rng, n) / np.float32(gs)).astype(np.float32)
        lr_t = float(np.float32(1e-3 * np.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step)))
        p0, m0, v0 = back(pd).copy(), back(md).copy(), back(vd).copy()
        K.adam_step(pd, fd(g), md, vd, lr_t, b1, b2, eps, gs)
        rp, rm, rv = F.adam(p0, g, m0, v0, lr_t, b1, b2, eps, gs)
        gg = np.abs(g.astype(np.float64)) * gs
        Bm = np.abs(b1 * m0.astype(np.float64)) + (1.0 - b1) * gg
        assert_bar(back(md), rm, F.bar32(4, Bm), "m, step %d" % step)
        assert_bar(back(vd), rv, F.bar32(7, rv), "v, step %d" % step)
        den = np.sqrt(rv) + eps
        u = lr_t * rm / den
        bar = F.bar32(4, Bm) * lr_t / den + F.bar32(7 + SQRTF, u) + F.bar32(1, np.abs(p0) + np.abs(u))
        assert_bar(back(pd), rp, bar, "p, step %d" % step)
        worst = max(worst, float((np.abs(back(pd) - rp) / bar).max()))
    print("\nobserved adam (sqrtf + division): %.3f of its bar" % worst)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5
SENTINEL = 1234.0


class Refusal:
    def __init__(self, lib, K):
        self.lib, self.K = lib, K
        self.out = []

    def buf(self, n):
        t = torch.full((n + 16,), SENTINEL, device="cuda", dtype=torch.float32)
        self.out.append(t)
        return t

    def refused(self, code, fn, *args):
        rc = getattr(self.lib, fn)(*args, self.K._stream())
        torch.cuda.synchronize()
        assert rc == code, (fn, rc, self.lib.shdr_last_error())
        for t in self.out:
            assert bool((t == SENTINEL).all()), fn + ": a refused call wrote to its output"


@pytest.fixture
def refusal(lib, K):
    return Refusal(lib, K)


def test_refusals_nhwc_family(refusal):
    r = refusal
    x = torch.ones(2 * 12 * 12 * 16 + 16, device="cuda")
    y = r.buf(2 * 12 * 12 * 16)
    for fn in ("shdr_avgpool2_fwd_f32", "shdr_maxpool2_fwd_f32", "shdr_maxpool3s2_fwd_f32", "shdr_resize2x_fwd_f32", "shdr_avgpool2_bwd_f32",
               "shdr_resize2x_bwd_f32", "shdr_upsample_zero2_f32"):
        r.refused(E_NULL, fn, None, P(y), 2, 6, 6, 8)
        r.refused(E_NULL, fn, P(x), None, 2, 6, 6, 8)
        r.refused(E_ALIGN, fn, P(x), P(y), 2, 6, 6, 6)                      # C % 4 != 0
        r.refused(E_ALIGN, fn, P(x, 4), P(y), 2, 6, 6, 8)                   # a pointer offset by one float
        r.refused(E_ALIGN, fn, P(x), P(y, 4), 2, 6, 6, 8)
        r.refused(E_SHAPE, fn, P(x), P(y), 0, 6, 6, 8)
    r.refused(E_SHAPE, "shdr_avgpool2_fwd_f32", P(x), P(y), 2, 1, 6, 8)     # nothing to pool
    r.refused(E_SHAPE, "shdr_maxpool2_fwd_f32", P(x), P(y), 2, 5, 6, 8)     # odd H
    r.refused(E_SHAPE, "shdr_maxpool2_fwd_f32", P(x), P(y), 2, 6, 5, 8)     # odd W
    r.refused(E_SHAPE, "shdr_maxpool2_bwd_f32", P(x), P(x), P(y), 2, 5, 6, 8)
    r.refused(E_SHAPE, "shdr_maxpool2_bwd_f32", P(x), P(x), P(y), 2, 6, 5, 8)
    r.refused(E_ALIGN, "shdr_maxpool2_bwd_f32", P(x), P(x), P(y), 2, 6, 6, 6)
    r.refused(E_NULL, "shdr_maxpool2_bwd_f32", P(x), None, P(y), 2, 6, 6, 8)
    r.refused(E_ALIGN, "shdr_maxpool2_bwd_f32", P(x), P(x, 4), P(y), 2, 6, 6, 8)     # dy offset by one float
    r.refused(E_ALIGN, "shdr_maxpool3s2_bwd_f32", P(x), P(x), P(x), P(y), 2, 6, 6, 6)
    r.refused(E_ALIGN, "shdr_maxpool3s2_bwd_f32", P(x), P(x), P(x), P(y, 4), 2, 6, 6, 8)
    r.refused(E_NULL, "shdr_maxpool3s2_bwd_f32", P(x), None, P(x), P(y), 2, 6, 6, 8)
    r.refused(E_NULL, "shdr_maxpool3s2_bwd_f32", P(x), P(x), None, P(y), 2, 6, 6, 8)
    r.refused(E_ALIGN, "shdr_maxpool3s2_bwd_f32", P(x), P(x, 4), P(x), P(y), 2, 6, 6, 8)   # y (the pooled output) offset by one float
    r.refused(E_ALIGN, "shdr_maxpool3s2_bwd_f32", P(x), P(x), P(x, 4), P(y), 2, 6, 6, 8)   # dy
    r.refused(E_ALIGN, "shdr_gap_fwd_f32", P(x), P(y), 2, 36, 6)
    r.refused(E_ALIGN, "shdr_gap_fwd_f32", P(x, 4), P(y), 2, 36, 8)
    r.refused(E_ALIGN, "shdr_gap_bwd_f32", P(x), P(y), 2, 36, 6)
    r.refused(E_ALIGN, "shdr_gap_bwd_f32", P(x), P(y, 4), 2, 36, 8)
    r.refused(E_NULL, "shdr_gap_bwd_f32", None, P(y), 2, 36, 8)


def test_refusals_act_bwd_bias_and_elementwise(refusal):
    r = refusal
    x = torch.ones(4 * 2048 + 16, device="cuda")
    dz, db, ws = r.buf(4 * 2048), r.buf(2048), r.buf(2048)
    f = "shdr_act_bwd_bias_f32"
    r.refused(E_SHAPE, f, P(x), P(x), P(dz), P(db), P(ws), 4, 12, 1)           # Q = 3: no power of two
    r.refused(E_SHAPE, f, P(x), P(x), P(dz), P(db), P(ws), 4, 2048, 1)         # Q = 512 > 256
    r.refused(E_SHAPE, f, P(x), P(x), P(dz), P(db), P(ws), 4, 6, 1)            # C % 4 != 0
    r.refused(E_SHAPE, f, P(x), P(x), P(dz), P(db), P(ws), 4, 8, 4)            # no such activation
    r.refused(E_ALIGN, f, P(x, 4), P(x), P(dz), P(db), P(ws), 4, 8, 1)
    r.refused(E_ALIGN, f, P(x), P(x, 4), P(dz), P(db), P(ws), 4, 8, 1)
    r.refused(E_ALIGN, f, P(x), P(x), P(dz, 4), P(db), P(ws), 4, 8, 1)
    r.refused(E_NULL, f, None, P(x), P(dz), P(db), P(ws), 4, 8, 1)
    r.refused(E_NULL, f, P(x), P(x), P(dz), None, P(ws), 4, 8, 1)
    for act in (1, 2, 3):
        r.refused(E_NULL, f, P(x), None, P(dz), P(db), P(ws), 4, 8, act)       # an activation but no y
        r.refused(E_NULL, f, P(x), P(x), None, P(db), P(ws), 4, 8, act)
    y = r.buf(64)
    r.refused(E_ALIGN, "shdr_clip_fwd_f32", P(x, 4), P(y), 16, 0.0, 1.0)
    r.refused(E_ALIGN, "shdr_clip_fwd_f32", P(x), P(y, 4), 16, 0.0, 1.0)
    r.refused(E_NULL, "shdr_clip_fwd_f32", None, P(y), 16, 0.0, 1.0)
    r.refused(E_NULL, "shdr_clip_bwd_f32", P(x), None, P(y), 16, 0.0, 1.0)
    r.refused(E_NULL, "shdr_logc_bwd_f32", P(x), P(x), None, 16)
    r.refused(E_SHAPE, "shdr_vgg_preprocess_fwd_f32", P(x), P(y), 4, 5)
    r.refused(E_ALIGN, "shdr_vgg_preprocess_fwd_f32", P(x), P(y, 4), 4, 4)
    r.refused(E_SHAPE, "shdr_vgg_preprocess_bwd_f32", P(x), P(y), 4, 5)
    r.refused(E_SHAPE, "shdr_reverse3_fwd_f32", P(x), P(x), 4)                  # in place
    r.refused(E_SHAPE, "shdr_alpha_blend_fwd_f32", P(x), P(x), P(y), None, 4, 0.0)
    r.refused(E_SHAPE, "shdr_alpha_mask_f32", P(x), P(y), 4, 0.0)
    r.refused(E_SHAPE, "shdr_pad_channels_f32", P(x), P(y), 4, 8, 4)            # Cout < Cin
    r.refused(E_SHAPE, "shdr_pack3_fwd_f32", P(x), P(x), None, None, 2, P(y), 5, 4)
    r.refused(E_NULL, "shdr_pack3_fwd_f32", P(x), None, None, None, 2, P(y), 8, 4)
    r.refused(E_SHAPE, "shdr_unpack3_f32", P(x), P(y), P(y), None, None, 2, 5, 4)
    r.refused(E_NULL, "shdr_unpack3_f32", P(x), P(y), None, None, None, 2, 8, 4)
    r.refused(E_NULL, "shdr_adam_f32", P(y), None, P(y), P(y), 16, 1e-3, 0.9, 0.999, 1e-7, 1.0)
    r.refused(E_NULL, "shdr_affine_act_f32", None, None, None, None, P(y), 4, 4, 0)


def test_refusals_crf_losses_batchnorm(refusal, K):
    r = refusal
    x = torch.ones(8192 + 16, device="cuda")
    y, z = r.buf(8192), r.buf(64)
    for k in (1, 4097):                                                         # K out of range
        r.refused(E_SHAPE, "shdr_increase_fwd_f32", P(x), P(y), 1, k)
        r.refused(E_SHAPE, "shdr_increase_bwd_f32", P(x), P(x), P(y), 1, k)
    for k in (1, 8193):
        r.refused(E_SHAPE, "shdr_apply_rf_bwd_f32", P(x), P(x), P(x), P(y), P(z), 1, 8, k)
    r.refused(E_SHAPE, "shdr_apply_rf_fwd_f32", P(x), P(x), P(y), 1, 8, 1)
    r.refused(E_SHAPE, "shdr_apply_rf_fwd_f32", P(x), P(x), P(y), 1, 8, 16385)
    r.refused(E_ALIGN, "shdr_apply_rf_fwd_f32", P(x, 4), P(x), P(y), 1, 8, 1024)       # n_per_batch % 4 == 0 takes float4s
    r.refused(E_NULL, "shdr_apply_rf_bwd_f32", P(x), P(x), P(x), None, P(z), 1, 8, 1024)
    # B > 65535 (the batch is gridDim.y)
    r.refused(E_SHAPE, "shdr_apply_rf_fwd_f32", P(x), P(x), P(y), 65536, 1, 2)
    r.refused(E_SHAPE, "shdr_apply_rf_bwd_f32", P(x), P(x), P(x), P(y), P(z), 65536, 1, 2)
    r.refused(E_SHAPE, "shdr_diff_loss_f32", P(x), P(x), P(y), 65536, 1, 0)
    r.refused(E_SHAPE, "shdr_sample_dot_f32", P(x), P(x), P(y), 65536, 1)
    r.refused(E_SHAPE, "shdr_diff_loss_f32", P(x), P(x), P(y), 2, 8, 2)                 # no such mode
    r.refused(E_SHAPE, "shdr_diff_loss_bwd_f32", P(x), P(x), P(x), P(y), 2, 8, 2, 0)
    r.refused(E_NULL, "shdr_diff_loss_bwd_f32", P(x), P(x), None, P(y), 2, 8, 0, 0)
    r.refused(E_SHAPE, "shdr_tv_loss_f32", P(x), P(y), 1, 0, 4, 3)
    r.refused(E_NULL, "shdr_tv_loss_bwd_f32", P(x), None, P(y), 1, 4, 4, 3, 0)
    r.refused(E_NULL, "shdr_mean_norm_fwd_f32", P(x), None, P(y), 2, 8, 1e-6, 0.5)
    r.refused(E_NULL, "shdr_mean_norm_bwd_f32", P(x), P(x), None, P(y), 2, 8, 1e-6, 0.5)
    r.refused(E_NULL, "shdr_invcrf_decode_bwd_f32", P(x), P(x), P(x), None, P(y), P(y), P(z), 1, 8, 1024)
    r.refused(E_SHAPE, "shdr_lin_frontend_bwd_f32", P(x), P(x), P(y), 1, 1, 4, 96)      # H < 2: no REFLECT padding
    r.refused(E_SHAPE, "shdr_lin_frontend_bwd_f32", P(x), P(x), P(y), 1, 4, 4, 92)
    r.refused(E_SHAPE, "shdr_soft_hist_bwd_f32", P(x), P(x), P(y), 4, 3, 0)
    ws = K._bn_ws(16, x.device)
    r.refused(E_NULL, "shdr_bn_stats_f32", P(x), P(ws), P(y), P(z), P(y), None, 64, 8, 0.99)        # moving stats come in pairs
    r.refused(E_NULL, "shdr_bn_stats_f32", P(x), None, P(y), P(z), None, None, 64, 8, 0.99)
    r.refused(E_SHAPE, "shdr_bn_stats_f32", P(x), P(ws), P(y), P(z), None, None, 0, 8, 0.99)
    r.refused(E_NULL, "shdr_bn_train_apply_f32", P(x), P(x), P(x), P(x), None, P(y), 64, 8, EPS, 1)
    r.refused(E_NULL, "shdr_bn_bwd_f32", P(x), P(x), None, P(x), P(x), P(x), None, P(y), P(z), P(y), 64, 8, EPS)
