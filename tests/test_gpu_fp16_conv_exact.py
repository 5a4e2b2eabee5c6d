"""The convolution kernels of the native-fp16 path (csrc/conv_f16.hip, conv_f16_patch.hip, conv_f16_w3.hip, wgrad_f16.hip,
wgrad_f16_alltaps.hip) against the float64 reference of tests/conv_ref.py, EXACTLY and element by element.

Inputs are small integers: x, x2, dz in [-2, 2], filters in {-1, 0, 1}, biases in [-3, 3], x2_scale a power of two (2^-8 where the
networks use 1/255; the second source then holds multiples of 2^8, so that the scaled source is again in [-2, 2]), folded-BN scales in
{0.5, 1, 2}, integer shifts and residuals.  Every product and every fp32 partial sum is then an integer below 2^24 and exact in ANY
order; every expected value is an integer of magnitude <= 2048 (or such an integer times the power of two of the case) and exact in the
fp16 output.  Neither operand rounding, nor the MFMA accumulation order, nor the fp32 atomics of the weight gradient, nor a split-K grid
that depends on the CU count can excuse a difference: every comparison is whole-tensor equality, and each test first asserts that
precondition on the reference alone.

Two values are not integers and are MODELLED, not excused (conv_ref.epilogue):
  leaky relu  the kernels form v * 0.1f in fp32 and cast the product: the reference does the same two roundings on the exact integer v;
  tanh        the fp32 head only: |got - tanh(ref)| <= one fp32 ulp of the result + the assumed tanhf bound TANHF of
              test_gpu_tape_f32.py; the worst observed distance is printed.  Where tanh meets an fp16 output (a layer the patch kernel
              declines) the test asserts that no tanh(ref) lies within that bound of an fp16 rounding boundary: the cast is then decided.

Outputs live in buffers with GUARD sentinel elements (an fp16 / fp32 NaN pattern) before and after the tensor, asserted untouched.  The
weight gradient is ACCUMULATED with atomics (`dw +=`, the caller zeroes it: include/shdr.h), so the elements of dw the ABI must not touch
-- columns >= cout_valid, rows of the other source -- hold a FINITE sentinel: a NaN would swallow a stray atomic add.

Calls: `_ops.pack_filter_h`, `_ops.conv2d_h` (its result must equal the guarded C-ABI call bit for bit), `_autograd._dgrad_h` for the
input gradient (its decompositions live in Python), and the C ABI where a wrapper hides a choice (c1_rows, dz_channels, accumulation,
alignment, the output buffer)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import conv_ref as C
from test_gpu_tape_f32 import TANHF

pytestmark = pytest.mark.gpu

GUARD = 64
SENT16 = 0x7E5A                       # an fp16 NaN pattern
SENT32 = 0x7FC5A5A5                   # an fp32 NaN pattern
FINITE = -12345.0                     # dw elements that only a stray atomic add could change
BOUND = 2048
NONE, RELU, LRELU, TANH = C.ACT_NONE, C.ACT_RELU, C.ACT_LRELU, C.ACT_TANH
S8 = 2.0 ** -8
E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


@pytest.fixture(scope="module")
def A(shdr):
    return importlib.import_module("singlehdr-tf2_amd._autograd")


# ---------------------------------------------------------------------------------------------------------------------------------
# operands, buffers, assertions
# ---------------------------------------------------------------------------------------------------------------------------------
def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def dev_ints(shape, lo, hi, seed):
    """integers generated on the device (the large cases); returns (fp16 device tensor, float64 host copy)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, device="cuda", generator=g, dtype=torch.int32).half()
    return t, t.cpu().numpy().astype(np.float64)


def h16(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a), "operand not exact in fp16"
    return torch.from_numpy(a.astype(np.float16)).cuda()


def f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def P(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def guarded(numel, half):
    """(whole buffer, view of `numel` elements between two GUARDs), filled with the sentinel; the view is 16-byte aligned"""
    buf = torch.full((numel + 2 * GUARD,), SENT16 if half else SENT32, device="cuda", dtype=torch.int16 if half else torch.int32)
    view = buf[GUARD:GUARD + numel]
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, numel, what):
    torch.cuda.synchronize()
    sent = SENT16 if buf.dtype == torch.int16 else SENT32
    assert bool((buf[:GUARD] == sent).all()), what + ": bytes BEFORE the tensor were written"
    assert bool((buf[GUARD + numel:] == sent).all()), what + ": bytes PAST the tensor were written"


def untouched(buf, what):
    torch.cuda.synchronize()
    sent = SENT16 if buf.dtype == torch.int16 else SENT32
    assert bool((buf == sent).all()), what + ": a refused call wrote its output"


def precondition(ref, step=1.0, what=""):
    """every expected value is an integer multiple of `step` of magnitude <= 2048 steps: exact in fp32 sums and in an fp16 output"""
    q = np.asarray(ref, dtype=np.float64) / step
    assert np.array_equal(q, np.rint(q)), what + ": reference is not a multiple of %g" % step
    assert float(np.abs(q).max(initial=0.0)) <= BOUND, what + ": |reference| = %g steps > %d" % (float(np.abs(q).max()), BOUND)


def bits16(a):
    """fp16 bit patterns with -0 mapped to +0"""
    b = np.ascontiguousarray(a).view(np.uint16).copy()
    b[b == 0x8000] = 0
    return b


def same(got, want, what, tile):
    """whole-tensor equality; on a difference the message names the first differing index, the tile it lies in (index // `tile`) and
    got / want there"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float16:
        g, w = bits16(got), bits16(want)
    else:
        g, w = got, want
    bad = g != w
    if bad.any():
        i = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        t = tuple(a // b for a, b in zip(i, tile))
        raise AssertionError("%s: %d of %d elements differ; first at %s, tile %s (tile shape %s): got %r, want %r"
                             % (what, int(bad.sum()), bad.size, i, t, tuple(tile), float(got[i]), float(want[i])))
    np.testing.assert_array_equal(g, w, err_msg=what)


def desc_of(K, x_shape, c2, khw, cout, stride, cout_valid=None, pad=None, out_hw=None, act1=NONE, act2=NONE):
    d = K._conv_desc_h(tuple(x_shape), c2, khw, cout, stride, cout_valid, pad, out_hw)
    d.act1, d.act2 = act1, act2
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def fwd_operands(seed, n, h, w, c1, c2, cout, khw, x2s, head):
    rng = np.random.default_rng(seed)
    x = ints(rng, (n, h, w, c1), -2, 2)
    x2 = ints(rng, (n, h, w, c2), -2, 2) / x2s if c2 else None           # the SCALED second source is in [-2, 2]
    wt = ints(rng, tuple(khw) + (c1 + c2, cout), -1, 1)                 # (a head keeps non-zero columns >= cout_valid: a stray store shows)
    b = ints(rng, (cout,), -3, 3)
    return rng, x, x2, wt, b


def run_fwd(K, lib, x, x2, wt, b, stride, act1, x2s=1.0, head=0, pad=None, out_hw=None, fused=None, what="fwd", wrapper=True):
    """shdr_conv2d_fwd_f16 / shdr_conv2d_fwd_fused_f16 into a guarded buffer -> host array (fp16, or fp32 [.., head] for a head).
    fused = dict(scale, shift, res, res_f32, act2)"""
    khw, cout = tuple(wt.shape[:2]), wt.shape[3]
    c1, c2 = x.shape[3], 0 if x2 is None else x2.shape[3]
    xd, x2d = h16(x), None if x2 is None else h16(x2)
    wp = K.pack_filter_h(f32(wt), c1, c2, x2s)
    bd = f32(b)
    f = fused or {}
    d = desc_of(K, x.shape, c2, khw, cout, stride, head or None, pad, out_hw, act1, f.get("act2", NONE))
    nch = head or cout
    numel = x.shape[0] * d.Ho * d.Wo * nch
    buf, y = guarded(numel, half=not head)
    if fused is None:
        rc = lib.shdr_conv2d_fwd_f16(ctypes.byref(d), P(xd), P(x2d), P(wp), P(bd), P(y), int(bool(head)), K._stream())
    else:
        res = f.get("res")
        resd = None
        if res is not None:
            resd = f32(res) if f["res_f32"] else h16(res)
            d.res_cstride = res.shape[3]
        scd, shd = f32(f.get("scale")), f32(f.get("shift"))
        rc = lib.shdr_conv2d_fwd_fused_f16(ctypes.byref(d), P(xd), P(x2d), P(wp), P(bd), P(scd), P(shd), P(resd), int(bool(f.get("res_f32"))),
                                           P(y), int(bool(head)), K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    guards_intact(buf, numel, what)
    shape = (x.shape[0], d.Ho, d.Wo, nch)
    got_t = (y.view(torch.float32) if head else y.view(torch.float16)).view(shape)
    if wrapper and fused is None:                                        # the _ops wrapper is the same call
        yy = K.conv2d_h(xd, wp, bd, khw, cout, stride=stride, x2=x2d, act1=act1, cout_valid=head or None, pad=pad, out_hw=out_hw)
        assert yy.dtype == got_t.dtype and tuple(yy.shape) == shape
        assert torch.equal(yy.view(torch.int32 if head else torch.int16), got_t.view(torch.int32 if head else torch.int16)), what + ": wrapper"
    return got_t.cpu().numpy()


def check_fwd(K, lib, seed, n, h, w, c1, c2, cout, khw, stride, act1, tile, x2s=1.0, head=0, pad=None, out_hw=None, fused=None,
              what="fwd", fused_spec=None):
    rng, x, x2, wt, b = fwd_operands(seed, n, h, w, c1, c2, cout, khw, x2s, head)
    z = C.conv2d(x, x2, wt, b, stride, x2s, pad, out_hw)
    precondition(z, 1.0, what + " z")
    if head:
        z = z[..., :head]
    f = None
    if fused_spec is not None:
        f = make_fused(rng, fused_spec, z.shape)
    fargs = {} if f is None else dict(scale=f.get("scale"), shift=f.get("shift"), residual=f.get("res"), act2=f.get("act2", NONE))
    want = C.epilogue(z, act1, **fargs)
    if act1 != LRELU and act1 != TANH and fargs.get("act2") != TANH:
        precondition(want, 0.5 if f and f.get("scale") is not None else 1.0, what + " y")
    got = run_fwd(K, lib, x, x2, wt, b, stride, act1, x2s, head, pad, out_hw, f, what)
    if TANH in (act1, fargs.get("act2")):
        return got, want, z
    same(got, want if head else C.to_f16(want), what, tile)
    return got, want, z


def make_fused(rng, spec, zshape):
    """spec: subset of {"scale", "shift", "res16", "res32", "act2"}"""
    c = zshape[-1]
    f = {}
    if "scale" in spec:
        f["scale"] = rng.choice([0.5, 1.0, 2.0], size=c)
    if "shift" in spec:
        f["shift"] = ints(rng, (c,), -5, 5)
    if "res16" in spec or "res32" in spec:
        f["res"] = ints(rng, tuple(zshape[:3]) + (c + 8,), -9, 9)       # res_cstride > the channel count
        f["res_f32"] = "res32" in spec
    if "act2" in spec:
        f["act2"] = RELU
    return f


def tanh_bar(t):
    """one fp32 ulp of the result + the assumed tanhf bound (TANHF units of 2^-24 relative to the result)"""
    t = np.abs(np.asarray(t, dtype=np.float64))
    return np.spacing(t.astype(np.float32)).astype(np.float64) + TANHF * 2.0 ** -24 * t


def check_tanh_head(got, z, what):
    t = np.tanh(z)
    err = np.abs(got.astype(np.float64) - t)
    bar = tanh_bar(t)
    print("\nobserved %s: worst |got - tanh(ref)| = %.3f of its bar" % (what, float((err / np.maximum(bar, 1e-300)).max())))
    bad = ~(err <= bar)
    assert not bad.any(), "%s: %d elements over the tanh bar, first at %s" % (what, int(bad.sum()), np.unravel_index(int(np.argmax(bad)), bad.shape))


# general implicit-GEMM kernel (SHDR_NO_PATCH=1, SHDR_NO_W3=1).  Tile forms by Cout: % 128 -> BM 128 (8 x 16 pixels), BN 128;
# % 64 -> BM 256 (16 x 16), BN 64; % 32 -> BN 32; else BN 16.  FAST k order iff (C1 + C2) % 32 == 0 and the sources split on a
# 32-channel boundary; KC = 2 chunks per stage unless nchunks == 1.
# id, n, h, w, c1, c2, cout, (kh, kw), stride, act1, x2s, head, pad, out_hw
GENERAL = [
    ("bn128_fast_3x3_32_odd_chunks", 2, 9, 17, 32, 0, 128, (3, 3), 1, RELU, 1.0, 0, None, None),           # 9 chunks: last stage of one
    ("bn128_two_n_blocks_1x1_64_256", 2, 7, 15, 64, 0, 256, (1, 1), 1, NONE, 1.0, 0, None, None),           # nblk_n = 2
    ("bn128_k4608_3x3_512", 2, 5, 7, 512, 0, 128, (3, 3), 1, NONE, 1.0, 0, None, None),                     # K = 4608, 144 chunks
    ("bn64_kc1_1x1_32", 2, 17, 33, 32, 0, 64, (1, 1), 1, LRELU, 1.0, 0, None, None),                        # nchunks == 1: KC = 1
    ("bn64_three_n_blocks_3x3_32_192", 2, 15, 16, 32, 0, 192, (3, 3), 1, LRELU, 1.0, 0, None, None),        # nblk_n = 3
    ("bn64_two_sources_64_64_scaled", 2, 16, 17, 64, 64, 64, (3, 3), 1, RELU, S8, 0, None, None),
    ("bn32_fast_3x3_64", 2, 17, 15, 64, 0, 32, (3, 3), 1, RELU, 1.0, 0, None, None),
    ("bn16_three_n_blocks_nat_24_48", 2, 16, 33, 24, 0, 48, (3, 3), 1, NONE, 1.0, 0, None, None),           # natural order, C1 = 24
    ("bn16_nat_c8_7x7_k_tail", 2, 17, 16, 8, 0, 16, (7, 7), 1, LRELU, 1.0, 0, None, None),                  # K = 392 = 12.25 chunks
    ("bn16_nat_16_16_scaled", 2, 15, 17, 16, 16, 16, (3, 3), 1, LRELU, S8, 0, None, None),
    ("bn32_nat_40_8", 2, 16, 15, 40, 8, 32, (3, 3), 1, RELU, S8, 0, None, None),
    ("bn64_nat_kc1_1x1_8", 2, 5, 33, 8, 0, 64, (1, 1), 1, NONE, 1.0, 0, None, None),                        # natural order, one chunk
    ("bn128_nat_c8_5x5", 2, 9, 16, 8, 0, 128, (5, 5), 1, RELU, 1.0, 0, None, None),                         # K = 200 = 6.25 chunks
    ("s2_1x1_even", 2, 16, 16, 32, 0, 64, (1, 1), 2, NONE, 1.0, 0, None, None),
    ("s2_1x1_odd", 2, 15, 17, 32, 0, 64, (1, 1), 2, RELU, 1.0, 0, None, None),
    ("s2_3x3_even", 2, 16, 34, 32, 0, 128, (3, 3), 2, RELU, 1.0, 0, None, None),
    ("s2_3x3_odd", 2, 15, 33, 32, 0, 16, (3, 3), 2, LRELU, 1.0, 0, None, None),
    ("s2_7x7_even_96", 2, 16, 18, 96, 0, 64, (7, 7), 2, NONE, 1.0, 0, None, None),                          # the Linearization-Net stem
    ("s2_7x7_odd_c8", 2, 17, 35, 8, 0, 32, (7, 7), 2, RELU, 1.0, 0, None, None),
    ("explicit_pad_4x3", 2, 9, 16, 32, 0, 64, (4, 3), 1, NONE, 1.0, 0, (2, 1), (10, 16)),                   # as the polyphase dgrad passes
    ("explicit_pad_2x2_nat", 2, 8, 17, 16, 0, 16, (2, 2), 1, NONE, 1.0, 0, (0, 1), (8, 18)),
    ("explicit_pad_3x4_bn128", 2, 8, 15, 64, 0, 128, (3, 4), 1, NONE, 1.0, 0, (1, 2), (9, 15)),
    ("head_f32_3_of_16", 2, 17, 18, 32, 0, 16, (3, 3), 1, NONE, 1.0, 3, None, None),
    ("head_f32_3_of_16_relu_nat", 2, 5, 33, 16, 0, 16, (3, 3), 1, RELU, 1.0, 3, None, None),
    ("head_f32_5_of_32_lrelu", 1, 16, 16, 32, 0, 32, (1, 1), 1, LRELU, 1.0, 5, None, None),
]
# spatial edges with N = 2 (the batch index takes part): W in {1, 15, 16, 17, 33} x H in {1, TH - 1, TH, TH + 1} for both TH
for _cout, _th in ((128, 8), (64, 16)):
    for _h in (1, _th - 1, _th, _th + 1):
        for _w in (1, 15, 16, 17, 33):
            GENERAL.append(("edges_bn%d_%dx%d" % (_cout, _h, _w), 2, _h, _w, 32, 0, _cout, (3, 3), 1, (RELU, NONE, LRELU)[(_h + _w) % 3],
                            1.0, 0, None, None))


def general_tile(cout):
    return (1, 8, 16, 128) if cout % 128 == 0 else (1, 16, 16, 64 if cout % 64 == 0 else 32 if cout % 32 == 0 else 16)


@pytest.mark.parametrize("case", GENERAL, ids=[c[0] for c in GENERAL])
def test_forward_general_kernel(K, lib, case, monkeypatch):
    name, n, h, w, c1, c2, cout, khw, stride, act1, x2s, head, pad, out_hw = case
    monkeypatch.setenv("SHDR_NO_PATCH", "1")
    monkeypatch.setenv("SHDR_NO_W3", "1")
    check_fwd(K, lib, len(name) * 131 + h * 17 + w, n, h, w, c1, c2, cout, khw, stride, act1, general_tile(cout), x2s, head, pad, out_hw,
              what=name)


def test_forward_general_kernel_tanh_head(K, lib, monkeypatch):
    """the one non-exact case: fp32 head, tanh of an exact integer accumulator"""
    monkeypatch.setenv("SHDR_NO_PATCH", "1")
    got, want, z = check_fwd(K, lib, 77, 2, 17, 18, 16, 0, 16, (3, 3), 1, TANH, general_tile(16), head=3, what="tanh head (general)")
    assert got.dtype == np.float32 and got.shape == z.shape
    check_tanh_head(got, z, "tanh head (general kernel)")


# patch kernel (default switches): one source of 8 / 16 / 32 channels or 16 + 16, Cout 16 / 32, k 3 / 5 / 7, stride 1, within LDS
# (every combination but 7x7 with 32 channels per pixel AND 32 couts)
SIZES = [(1, 1), (15, 33), (16, 16), (17, 15), (33, 17), (1, 17), (16, 1), (15, 16), (33, 33), (17, 1)]
PATCH = []
for _i, (_c1, _c2) in enumerate(((8, 0), (16, 0), (32, 0), (16, 16))):
    for _j, _cout in enumerate((16, 32)):
        for _l, _k in enumerate((3, 5, 7)):
            if _k == 7 and _c1 + _c2 == 32 and _cout == 32:
                continue                                                 # 100 KB filter + two patches: over the LDS limit (refused, below)
            _h, _w = SIZES[(_i * 6 + _j * 3 + _l) % len(SIZES)]
            _head = 3 if (_i + _j + _l) % 2 else 0                       # both output types
            PATCH.append(("patch_%d+%d_%d_k%d_%dx%d_%s" % (_c1, _c2, _cout, _k, _h, _w, "f32" if _head else "f16"), 2, _h, _w, _c1, _c2,
                          _cout, _k, (NONE, RELU, LRELU)[(_i + _l) % 3], _head))


@pytest.mark.parametrize("case", PATCH, ids=[c[0] for c in PATCH])
def test_forward_patch_kernel(K, lib, case):
    name, n, h, w, c1, c2, cout, k, act1, head = case
    d = desc_of(K, (n, h, w, c1), c2, (k, k), cout, 1, head or None)
    assert lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 1, "the case must reach the patch kernel"
    check_fwd(K, lib, len(name) * 37 + k, n, h, w, c1, c2, cout, (k, k), 1, act1, (1, 16, 16, cout), S8 if c2 else 1.0, head, what=name)


def test_forward_patch_kernel_tanh_head(K, lib):
    d = desc_of(K, (2, 17, 33, 16), 0, (3, 3), 16, 1, 3)
    assert lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 1
    got, want, z = check_fwd(K, lib, 78, 2, 17, 33, 16, 0, 16, (3, 3), 1, TANH, (1, 16, 16, 16), head=3, what="tanh head (patch)")
    check_tanh_head(got, z, "tanh head (patch kernel)")


@pytest.mark.parametrize("c1,c2,cout", [(32, 0, 32), (16, 16, 32)])
def test_forward_patch_refused_7x7_32_lands_on_general_kernel(K, lib, c1, c2, cout):
    d = desc_of(K, (2, 17, 33, c1), c2, (7, 7), cout, 1)
    assert lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 0            # filter + two patches over the LDS limit
    check_fwd(K, lib, 79 + c2, 2, 17, 33, c1, c2, cout, (7, 7), 1, LRELU, general_tile(cout), S8 if c2 else 1.0, what="7x7 32 ch")


def test_forward_patch_refused_tanh_fp16_lands_on_general_kernel(K, lib):
    """tanh is compiled into the fp32-output path of the patch kernel only: with an fp16 output the layer runs on the general kernel.
    The cast is decided wherever tanh(ref) is further from an fp16 rounding boundary than the tanh bar: asserted on the reference."""
    d = desc_of(K, (2, 15, 17, 16), 0, (3, 3), 16, 1)
    assert lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 1            # the shape is the patch kernel's; the dispatcher declines for tanh
    got, want, z = check_fwd(K, lib, 80, 2, 15, 17, 16, 0, 16, (3, 3), 1, TANH, general_tile(16), what="tanh fp16")
    t = np.tanh(z)
    lo, hi = C.to_f16(t - tanh_bar(t)), C.to_f16(t + tanh_bar(t))
    assert np.array_equal(bits16(lo), bits16(hi)), "a tanh(ref) lies within the tanh bar of an fp16 rounding boundary: pick another seed"
    same(got, C.to_f16(t), "tanh fp16", general_tile(16))


# w3 kernel (SHDR_W3_MIN_BLOCKS=0): 3x3 / 1, C1 % 32 == C2 % 32 == 0, Cout % 64 == 0, 16 x 16 pixel tiles x 64 couts
W3 = [
    ("w3_32_64_17x31", 2, 17, 31, 32, 0, 64, RELU),
    ("w3_64_128_1x1", 2, 1, 1, 64, 0, 128, LRELU),
    ("w3_96_192_16x16", 2, 16, 16, 96, 0, 192, RELU),
    ("w3_96_64_17x31", 1, 17, 31, 96, 0, 64, LRELU),
    ("w3_32_32_128_17x31_scaled", 2, 17, 31, 32, 32, 128, LRELU),
    ("w3_64_64_64_16x16_scaled", 2, 16, 16, 64, 64, 64, RELU),
    ("w3_64_64_192_1x1_scaled", 2, 1, 1, 64, 64, 192, NONE),
    ("w3_32_192_31x17", 2, 31, 17, 32, 0, 192, NONE),
]


@pytest.mark.parametrize("case", W3, ids=[c[0] for c in W3])
def test_forward_w3_kernel(K, lib, case, monkeypatch):
    name, n, h, w, c1, c2, cout, act1 = case
    monkeypatch.setenv("SHDR_W3_MIN_BLOCKS", "0")
    d = desc_of(K, (n, h, w, c1), c2, (3, 3), cout, 1, act1=act1)
    assert lib.shdr_conv2d_w3_ok_f16(ctypes.byref(d)) == 1 and lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 0
    check_fwd(K, lib, len(name) * 53 + h, n, h, w, c1, c2, cout, (3, 3), 1, act1, (1, 16, 16, 64), S8 if c2 else 1.0, what=name)


# fused inference epilogue: y = act2(act1(z) * scale + shift + residual)
FUSED_OPTIONS = [("scale_shift", ("scale", "shift")), ("shift_only", ("shift",)), ("res16", ("res16",)), ("res32", ("res32",)),
                 ("act2_relu", ("shift", "act2")), ("all_res16", ("scale", "shift", "res16", "act2")),
                 ("all_res32", ("scale", "shift", "res32", "act2"))]
# family, n, h, w, c1, c2, cout, head, act1, env
FUSED_FAMILIES = [
    ("patch_head", 2, 17, 33, 16, 0, 16, 3, NONE, {}),                                  # fused patch kernel: fp32 head, 3x3, Cout 16
    ("patch_head_two_sources", 1, 15, 16, 16, 16, 16, 3, RELU, {}),
    ("w3", 2, 17, 31, 32, 32, 64, 0, RELU, {"SHDR_W3_MIN_BLOCKS": "0"}),                # fused w3 kernel; a residual -> general kernel
    ("general_bn128", 2, 9, 17, 32, 0, 128, 0, LRELU, {"SHDR_NO_W3": "1"}),
    ("general_bn16_nat", 2, 17, 15, 24, 0, 16, 0, RELU, {"SHDR_NO_PATCH": "1"}),
    ("general_head", 2, 16, 17, 32, 0, 16, 3, RELU, {"SHDR_NO_PATCH": "1"}),
]


@pytest.mark.parametrize("option", FUSED_OPTIONS, ids=[o[0] for o in FUSED_OPTIONS])
@pytest.mark.parametrize("family", FUSED_FAMILIES, ids=[f[0] for f in FUSED_FAMILIES])
def test_forward_fused_epilogue(K, lib, family, option, monkeypatch):
    fam, n, h, w, c1, c2, cout, head, act1, env = family
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    spec = option[1]
    has_res = "res16" in spec or "res32" in spec
    d = desc_of(K, (n, h, w, c1), c2, (3, 3), cout, 1, head or None, act1=act1)
    if fam.startswith("patch"):
        assert lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 1 and head and cout == 16
        tile = (1, 16, 16, 16)
    elif fam == "w3":
        assert lib.shdr_conv2d_w3_ok_f16(ctypes.byref(d)) == 1
        tile = general_tile(cout) if has_res else (1, 16, 16, 64)        # the fused w3 kernel declines a residual
    else:
        tile = general_tile(cout)
    check_fwd(K, lib, len(fam) * 19 + len(option[0]), n, h, w, c1, c2, cout, (3, 3), 1, act1, tile, S8 if c2 else 1.0, head,
              what=fam + " " + option[0], fused_spec=spec)


# ---------------------------------------------------------------------------------------------------------------------------------
# input gradient (through _autograd._dgrad_h: stride 1 = one conv on dz with the flipped / transposed filter; 1x1 / 2 = that on the
# coarse grid + upsample_zero2; k x k / 2 = four polyphase convs with explicit pad / out_hw)
# ---------------------------------------------------------------------------------------------------------------------------------
# id, n, h, w, cin_total, c_begin, c_count, cz (dz channels), cols (filter columns), k, stride, scale
DGRAD = [
    ("s1_1x1", 2, 15, 17, 32, 0, 32, 64, 64, 1, 1, 1.0),
    ("s1_3x3", 2, 17, 33, 16, 0, 16, 32, 32, 3, 1, 1.0),
    ("s1_3x3_wide", 2, 9, 16, 128, 0, 128, 64, 64, 3, 1, 1.0),
    ("s1_5x5", 2, 16, 15, 32, 0, 32, 16, 16, 5, 1, 1.0),
    ("s1_7x7", 1, 17, 16, 16, 0, 16, 16, 16, 7, 1, 1.0),
    ("s2_1x1_even", 2, 16, 18, 64, 0, 64, 128, 128, 1, 2, 1.0),
    ("s2_1x1_odd", 2, 15, 17, 64, 0, 64, 128, 128, 1, 2, 1.0),
    ("s2_3x3_even", 2, 16, 18, 32, 0, 32, 64, 64, 3, 2, 1.0),
    ("s2_3x3_odd", 2, 15, 17, 32, 0, 32, 64, 64, 3, 2, 1.0),
    ("s2_3x3_odd_even", 1, 17, 16, 16, 0, 16, 16, 16, 3, 2, 1.0),
    ("s2_7x7_even", 2, 16, 18, 96, 0, 96, 64, 64, 7, 2, 1.0),
    ("s2_7x7_odd", 2, 15, 17, 96, 0, 96, 64, 64, 7, 2, 1.0),
    ("s2_7x7_even_odd", 1, 18, 15, 16, 0, 16, 32, 32, 7, 2, 1.0),
    ("slice_c_begin_scaled", 2, 17, 15, 48, 32, 16, 16, 16, 3, 1, S8),                 # second source of 32 + 16, scale 2^-8
    ("slice_c_begin_scaled_wide", 2, 16, 17, 128, 64, 64, 64, 64, 3, 1, S8),
    ("slice_c_begin_scaled_s2", 1, 15, 17, 64, 32, 32, 32, 32, 3, 2, S8),
    ("head_dz_8_of_3", 2, 17, 33, 16, 0, 16, 8, 3, 3, 1, 1.0),                          # dz carries 8 channels, the filter 3 columns
    ("head_dz_8_of_3_wide", 2, 16, 15, 64, 0, 64, 8, 3, 3, 1, 1.0),
]


@pytest.mark.parametrize("case", DGRAD, ids=[c[0] for c in DGRAD])
def test_input_gradient(K, A, case):
    name, n, h, w, cin, c_begin, c_count, cz, cols, k, stride, scale = case
    rng = np.random.default_rng(len(name) * 29 + h)
    wt = ints(rng, (k, k, cin, cols), -1, 1)
    ho, wo = -(-h // stride), -(-w // stride)
    dz = ints(rng, (n, ho, wo, cz), -2, 2)                               # channels >= cols are NOT zero: they must be ignored
    x_shape = (n, h, w, c_count)
    ref = C.dgrad(dz, wt, x_shape, c_begin, c_count, scale, stride)
    precondition(ref, scale, name)
    got = A._dgrad_h(h16(dz), f32(wt), c_begin, c_count, scale, stride, x_shape)
    torch.cuda.synchronize()
    assert got.dtype == torch.float16 and tuple(got.shape) == x_shape
    same(got.cpu().numpy(), C.to_f16(ref), name, (1, 16 * stride, 16 * stride, 16))


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def run_wgrad(K, lib, x, x2, dz, k, stride, x2s, c1_rows=None, c2_rows=None, cout_valid=None, row_len=None, accumulate=False,
              what="wgrad", tile=(1, 1, 16, 16), xd=None, x2d=None, dzd=None):
    """shdr_conv2d_wgrad_f16 through the C ABI into a guarded dw [k, k, c1_rows + c2_rows, row_len] whose valid elements start at zero (or
    at integers: `accumulate`) and whose other elements hold FINITE; source 0 first, then source 1; whole-tensor equality at the end"""
    c1, c2 = x.shape[3], 0 if x2 is None else x2.shape[3]
    czc = dz.shape[3]
    c1_rows = c1 if c1_rows is None else c1_rows
    c2_rows = c2 if c2_rows is None else c2_rows
    row_len = czc if row_len is None else row_len
    cv = row_len if cout_valid is None else cout_valid
    ref = C.wgrad(x, x2, dz[..., :cv], (k, k, c1 + c2, cv), stride, x2s, None)
    precondition(ref, 1.0, what)
    rows = c1_rows + c2_rows
    init = np.full((k, k, rows, row_len), FINITE, dtype=np.float32)
    rng = np.random.default_rng(rows * 7 + row_len)
    init[:, :, :, :cv] = ints(rng, (k, k, rows, cv), -50, 50) if accumulate else 0.0
    want = init.copy()
    want[:, :, :c1_rows, :cv] += ref[:, :, :c1_rows].astype(np.float32)
    want_after_first = want.copy()
    if c2:
        want[:, :, c1_rows:, :cv] += ref[:, :, c1:c1 + c2_rows].astype(np.float32)
    numel = init.size
    buf, v = guarded(numel, half=False)
    dw = v.view(torch.float32).view(init.shape)
    dw.copy_(torch.from_numpy(init))
    xd = h16(x) if xd is None else xd
    dzd = h16(dz) if dzd is None else dzd
    d = desc_of(K, x.shape, c2, (k, k), row_len, stride, cv)
    d.x2_scale = x2s
    assert tuple(dz.shape[:3]) == (x.shape[0], d.Ho, d.Wo)
    rc = lib.shdr_conv2d_wgrad_f16(ctypes.byref(d), P(xd), 0, P(dzd), czc, c1_rows, c2_rows, P(dw), K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    guards_intact(buf, numel, what)
    same(dw.cpu().numpy(), want_after_first, what + " (source 0; the rows of source 1 and the columns >= cout_valid untouched)", tile)
    if c2:
        x2d = h16(x2) if x2d is None else x2d
        rc = lib.shdr_conv2d_wgrad_f16(ctypes.byref(d), P(x2d), 1, P(dzd), czc, c1_rows, c2_rows, P(dw), K._stream())
        assert rc == 0, (what, rc, lib.shdr_last_error())
        guards_intact(buf, numel, what)
        same(dw.cpu().numpy(), want, what + " (source 1)", tile)
    return d


def wgrad_operands(seed, n, h, w, c1, c2, cz, k, stride, x2s):
    rng = np.random.default_rng(seed)
    x = ints(rng, (n, h, w, c1), -2, 2)
    x2 = ints(rng, (n, h, w, c2), -2, 2) / x2s if c2 else None
    dz = ints(rng, (n, -(-h // stride), -(-w // stride), cz), -2, 2)
    return x, x2, dz


# per-tap kernel (SHDR_NO_ALLTAPS=1).  Dispatch (wgrad_f16.hip): CI_T by Cx -- % 128 -> 128; == 96 with Cz % 64 == 0 -> 96 (x CO_T 64);
# % 64 -> 64; % 32 -> 32; else 16 -- and CO_T by Cz -- % 128 -> 128; % 64 -> 64; % 32 -> 32; else 16.  With SHDR_WGRAD_256_MIN_PIXELS=0 the
# 8-wave forms come first: Cx % 256 == Cz % 256 == 0 -> 256 x 256; Cx % 256, Cz % 128 and not 1x1 -> 256 x 128; Cx % 128, Cz % 256 and not
# 1x1 -> 128 x 256.  KC = 4 chunks of 32 pixels per stage when CI_T + CO_T <= 128, else 2; a slice is a multiple of KC * 32 pixels and
# holds >= 1024 pixels when there are >= 2048.
# id, n, h, w, c1, c2, cz, k, stride, x2s, (CI_T, CO_T) the case reaches, opts
TAP = []
for _cx, _cit in ((128, 128), (64, 64), (32, 32), (16, 16)):
    for _cz, _cot in ((128, 128), (64, 64), (32, 32), (16, 16)):
        _h, _w = SIZES[(len(TAP) * 3 + 1) % len(SIZES)]
        TAP.append(("tile_%dx%d_%dx%d" % (_cit, _cot, _h, _w), 2, _h, _w, _cx, 0, _cz, 3, 1, 1.0, (_cit, _cot), {}))
TAP += [
    ("tile_96x64_stem_7x7s2", 2, 15, 17, 96, 0, 64, 7, 2, 1.0, (96, 64), {}),                       # Cx == 96 with Cz % 64 == 0
    ("tile_32x32_cx96_cz32", 1, 16, 17, 96, 0, 32, 3, 1, 1.0, (32, 32), {}),                        # Cx == 96 but Cz % 64 != 0: three 32-row tiles
    ("tile_256x256", 1, 6, 7, 256, 0, 256, 3, 1, 1.0, (256, 256), {"w256": True}),
    ("tile_256x256_two_ci_tiles_1x1", 1, 9, 8, 512, 0, 256, 1, 1, 1.0, (256, 256), {"w256": True}),   # 1x1 keeps the 256 x 256 form
    ("tile_256x128", 1, 7, 6, 256, 0, 128, 3, 1, 1.0, (256, 128), {"w256": True}),
    ("tile_128x256", 1, 5, 9, 128, 0, 256, 3, 1, 1.0, (128, 256), {"w256": True}),
    ("tile_1x1_excluded_256x128", 1, 7, 6, 256, 0, 128, 1, 1, 1.0, (128, 128), {"w256": True}),     # 1x1: 128 x 128 instead
    ("tile_1x1_excluded_128x256", 1, 5, 9, 128, 0, 256, 1, 1, 1.0, (128, 128), {"w256": True}),
    ("tile_256_below_threshold", 1, 6, 7, 256, 0, 256, 3, 1, 1.0, (128, 128), {}),                  # default threshold: 42 pixels < 4096
    ("ragged_cx8_dz8", 2, 5, 7, 8, 0, 8, 3, 1, 1.0, (16, 16), {}),
    ("ragged_cx24_dz24", 2, 7, 5, 24, 0, 24, 3, 1, 1.0, (16, 16), {}),
    ("ragged_cx40_dz8", 2, 6, 6, 40, 0, 8, 3, 1, 1.0, (16, 16), {}),
    ("ragged_cx8_dz24_7x7", 1, 9, 11, 8, 0, 24, 7, 1, 1.0, (16, 16), {}),
    ("rows_3_of_8_cols_3_of_16", 2, 9, 7, 8, 0, 16, 3, 1, 1.0, (16, 16), {"c1_rows": 3, "cout_valid": 3}),
    ("head_dz8_cols_3_rowlen_16", 2, 9, 7, 16, 0, 8, 3, 1, 1.0, (16, 16), {"cout_valid": 3, "row_len": 16}),   # as Conv2dHFn's head backward
    ("cols_3_of_16_wide_tile", 1, 8, 8, 64, 0, 16, 3, 1, 1.0, (64, 16), {"cout_valid": 3}),
    ("pixels_1", 1, 1, 1, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),
    ("pixels_31", 1, 1, 31, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),                                    # less than one chunk
    ("pixels_33", 1, 3, 11, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),
    ("pixels_129_kc4", 1, 3, 43, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),                               # KC * 32 + 1, KC = 4
    ("pixels_65_kc2", 1, 5, 13, 128, 0, 128, 3, 1, 1.0, (128, 128), {}),                            # KC * 32 + 1, KC = 2
    ("pixels_2115_two_slices", 1, 47, 45, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),                      # 1152 + 963: the last slice ragged
    ("pixels_2115_two_slices_kc2", 1, 47, 45, 128, 0, 64, 3, 1, 1.0, (128, 64), {}),                # 1088 + 1027
    ("pixels_23040_many_slices", 4, 72, 80, 32, 0, 32, 3, 1, 1.0, (32, 32), {"device": True}),
    ("k1", 2, 15, 17, 64, 0, 32, 1, 1, 1.0, (64, 32), {}),
    ("k7", 1, 16, 15, 16, 0, 16, 7, 1, 1.0, (16, 16), {}),
    ("k7_c8_stem", 2, 17, 16, 8, 0, 16, 7, 1, 1.0, (16, 16), {}),
    ("s2_1x1_odd", 2, 15, 17, 64, 0, 128, 1, 2, 1.0, (64, 128), {}),
    ("s2_3x3_odd", 2, 15, 17, 32, 0, 64, 3, 2, 1.0, (32, 64), {}),
    ("s2_3x3_odd_even", 2, 17, 16, 16, 0, 16, 3, 2, 1.0, (16, 16), {}),
    ("two_sources_32_32_scaled", 2, 17, 15, 32, 32, 64, 3, 1, S8, (32, 64), {}),
    ("two_sources_16_16_scaled", 2, 15, 16, 16, 16, 16, 3, 1, S8, (16, 16), {}),
    ("two_sources_40_8_scaled_rows", 1, 16, 17, 40, 8, 32, 3, 1, S8, (16, 32), {"c2_rows": 3}),     # x2 = a zero-padded 3-channel image
    ("two_sources_64_64_1x1_scaled", 2, 16, 16, 64, 64, 64, 1, 1, S8, (64, 64), {}),
    ("accumulate_32x32", 2, 17, 15, 32, 0, 32, 3, 1, 1.0, (32, 32), {"accumulate": True}),
    ("accumulate_two_sources", 1, 15, 17, 32, 32, 16, 3, 1, S8, (32, 16), {"accumulate": True}),
]


def run_wgrad_case(K, lib, case):
    name, n, h, w, c1, c2, cz, k, stride, x2s, tile, o = case
    seed = len(name) * 41 + h * 3 + w
    kw = dict(c1_rows=o.get("c1_rows"), c2_rows=o.get("c2_rows"), cout_valid=o.get("cout_valid"), row_len=o.get("row_len"),
              accumulate=o.get("accumulate", False), what=name, tile=(1, 1) + tuple(tile))
    if o.get("device"):
        xd, x = dev_ints((n, h, w, c1), -2, 2, seed)
        dzd, dz = dev_ints((n, h, w, cz), -2, 2, seed + 1)
        return run_wgrad(K, lib, x, None, dz, k, stride, x2s, xd=xd, dzd=dzd, **kw)
    x, x2, dz = wgrad_operands(seed, n, h, w, c1, c2, cz, k, stride, x2s)
    return run_wgrad(K, lib, x, x2, dz, k, stride, x2s, **kw)


@pytest.mark.parametrize("case", TAP, ids=[c[0] for c in TAP])
def test_weight_gradient_per_tap_kernel(K, lib, case, monkeypatch):
    monkeypatch.setenv("SHDR_NO_ALLTAPS", "1")
    if case[11].get("w256"):
        monkeypatch.setenv("SHDR_WGRAD_256_MIN_PIXELS", "0")
    run_wgrad_case(K, lib, case)


# all-taps kernel (SHDR_ALLTAPS_MIN_PIXELS=0): every (k, cx, dz_channels) of its predicate; instantiations <KK, CI_T, CO_T, MODE>:
# k 7 -> <7,16,16,0>; k 5 -> <5,cx,cz,0>; k 3 -> CI_T = 64 (cx % 64 == 0) / 32 / 16 (cx 8, 16), CO_T = 64 / 32 / 16 (cz 8, 16), MODE 1 for 64 x 64
ALLTAPS_SIZES = [(1, 1, 1), (1, 5, 70), (1, 33, 50), (2, 40, 72)]
ALLTAPS = []
for _k, _cxs, _czs in ((3, (8, 16, 32, 64, 128), (8, 16, 32, 64)), (5, (16, 32), (16, 32)), (7, (8, 16), (16,))):
    for _cx in _cxs:
        for _cz in _czs:
            _n, _h, _w = ALLTAPS_SIZES[len(ALLTAPS) % 4]
            _cit = 64 if _cx % 64 == 0 else 32 if _cx == 32 else 16
            _cot = 64 if _cz == 64 else 32 if _cz == 32 else 16
            ALLTAPS.append(("alltaps_k%d_%d_%d_%dx%dx%d" % (_k, _cx, _cz, _n, _h, _w), _n, _h, _w, _cx, 0, _cz, _k, 1, 1.0, (_cit, _cot), {}))
ALLTAPS += [
    ("alltaps_mode1_64_64_2x40x72", 2, 40, 72, 64, 0, 64, 3, 1, 1.0, (64, 64), {}),
    ("alltaps_mode1_128_64_5x70", 1, 5, 70, 128, 0, 64, 3, 1, 1.0, (64, 64), {}),
    ("alltaps_k7_8_16_2x40x72", 2, 40, 72, 8, 0, 16, 7, 1, 1.0, (16, 16), {}),
    ("alltaps_k5_32_32_33x50", 1, 33, 50, 32, 0, 32, 5, 1, 1.0, (32, 32), {}),
    ("alltaps_two_sources_32_32_scaled", 1, 33, 50, 32, 32, 32, 3, 1, S8, (32, 32), {}),
    ("alltaps_two_sources_16_16_k5_accumulate", 1, 5, 70, 16, 16, 16, 5, 1, S8, (16, 16), {"accumulate": True}),
    ("alltaps_rows_3_of_8_cols_3_of_16_k7", 1, 33, 50, 8, 0, 16, 7, 1, 1.0, (16, 16), {"c1_rows": 3, "cout_valid": 3}),
    ("alltaps_head_dz8_cols_3_rowlen_16", 2, 40, 72, 16, 0, 8, 3, 1, 1.0, (16, 16), {"cout_valid": 3, "row_len": 16}),
]


@pytest.mark.parametrize("case", ALLTAPS, ids=[c[0] for c in ALLTAPS])
def test_weight_gradient_all_taps_kernel(K, lib, case, monkeypatch):
    monkeypatch.setenv("SHDR_ALLTAPS_MIN_PIXELS", "0")
    d = run_wgrad_case(K, lib, case)
    assert lib.shdr_conv2d_wgrad_alltaps_ok_f16(ctypes.byref(d), 0, case[6]) == 1, "the case must reach the all-taps kernel"
    if case[5]:
        assert lib.shdr_conv2d_wgrad_alltaps_ok_f16(ctypes.byref(d), 1, case[6]) == 1


def test_weight_gradient_all_taps_refuses_cx256_and_per_tap_kernel_runs(K, lib, monkeypatch):
    monkeypatch.setenv("SHDR_ALLTAPS_MIN_PIXELS", "0")
    case = ("alltaps_refused_cx256", 1, 5, 70, 256, 0, 64, 3, 1, 1.0, (128, 64), {})
    d = run_wgrad_case(K, lib, case)
    assert lib.shdr_conv2d_wgrad_alltaps_ok_f16(ctypes.byref(d), 0, 64) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: argument checks only -- every pointer handed over is a valid, large enough buffer
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(K, lib):
    n, h, w, c1, cout = 1, 8, 8, 32, 64
    x = torch.zeros((n * h * w * c1 + 64,), device="cuda", dtype=torch.float16)
    x2 = torch.zeros_like(x)
    wp = torch.zeros((9 * 64 * 64 * 2 + 64,), device="cuda", dtype=torch.float16)
    bias = torch.zeros((cout + 16,), device="cuda", dtype=torch.float32)
    res = torch.zeros((n * h * w * 2 * cout,), device="cuda", dtype=torch.float16)
    ybuf, y = guarded(n * h * w * 2 * cout, half=True)
    dwbuf, dw = guarded(9 * 64 * 64, half=False)
    st = K._stream()

    def desc(**kw):
        d = desc_of(K, (n, h, w, kw.pop("c1", c1)), kw.pop("c2", 0), kw.pop("khw", (3, 3)), kw.pop("cout", cout), kw.pop("stride", 1))
        for k_, v_ in kw.items():
            setattr(d, k_, v_)
        return d

    def refused(rc, code, what):
        assert rc == code, (what, rc, code, lib.shdr_last_error())
        untouched(ybuf, what)
        untouched(dwbuf, what)

    fwd = lib.shdr_conv2d_fwd_f16
    # misaligned pointers, each in turn (8 bytes past a 16-byte boundary)
    for i, what in enumerate(("x1", "x2", "wp", "bias", "y")):
        d = desc(c2=32)
        args = [P(x), P(x2), P(wp), P(bias), P(y)]
        args[i] = P((x, x2, wp, bias, y)[i], 8)
        refused(fwd(ctypes.byref(d), *args, 0, st), E_ALIGN, "fwd misaligned " + what)
    d = desc(c1=16, cout=16)                                             # the patch kernel's own entry
    assert lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 1
    refused(lib.shdr_conv2d_fwd_patch_f16(ctypes.byref(d), P(x, 8), None, P(wp), P(bias), P(y), 0, st), E_ALIGN, "patch misaligned x1")
    refused(lib.shdr_conv2d_fwd_patch_f16(ctypes.byref(d), P(x), None, P(wp), P(bias), P(y, 8), 0, st), E_ALIGN, "patch misaligned y")
    refused(lib.shdr_conv2d_fwd_patch_f16(ctypes.byref(desc(c1=16, cout=16, act1=TANH)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE,
            "patch entry: tanh with an fp16 output")
    refused(lib.shdr_conv2d_fwd_patch_f16(ctypes.byref(desc(c1=64, cout=16)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE,
            "patch entry: a shape it does not take")
    refused(lib.shdr_conv2d_fwd_w3_f16(ctypes.byref(desc(stride=2)), P(x), None, P(wp), P(bias), P(y), st), E_SHAPE,
            "w3 entry: a shape it does not take")
    # shapes
    refused(fwd(ctypes.byref(desc(c1=12)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE, "C1 % 8")
    refused(fwd(ctypes.byref(desc(c2=12)), P(x), P(x2), P(wp), P(bias), P(y), 0, st), E_SHAPE, "C2 % 8")
    refused(fwd(ctypes.byref(desc(cout=24)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE, "Cout % 16")
    refused(fwd(ctypes.byref(desc(pad_t=3)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE, "pad_t outside the kernel")
    refused(fwd(ctypes.byref(desc(pad_l=-1)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE, "negative pad_l")
    refused(fwd(ctypes.byref(desc(Ho=h + 2)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE, "output too large for the input")
    refused(fwd(ctypes.byref(desc(cout_valid=3)), P(x), None, P(wp), P(bias), P(y), 0, st), E_SHAPE, "cout_valid < Cout with an fp16 output")
    refused(fwd(ctypes.byref(desc(c2=32)), P(x), None, P(wp), P(bias), P(y), 0, st), E_NULL, "C2 > 0 without x2")
    refused(fwd(ctypes.byref(desc()), P(x), P(x2), P(wp), P(bias), P(y), 0, st), E_NULL, "x2 without C2")
    # fused entry
    fused = lib.shdr_conv2d_fwd_fused_f16
    refused(fused(ctypes.byref(desc(res_cstride=cout - 8)), P(x), None, P(wp), P(bias), None, None, P(res), 0, P(y), 0, st), E_SHAPE,
            "res_cstride too small")
    refused(fused(ctypes.byref(desc(act2=TANH)), P(x), None, P(wp), P(bias), None, P(bias), None, 0, P(y), 0, st), E_SHAPE,
            "fused: tanh with an fp16 output")
    # weight gradient
    wg = lib.shdr_conv2d_wgrad_f16
    refused(wg(ctypes.byref(desc()), P(x), 1, P(x2), cout, c1, 0, P(dw), st), E_SHAPE, "which = 1 without x2")
    refused(wg(ctypes.byref(desc()), P(x), 2, P(x2), cout, c1, 0, P(dw), st), E_SHAPE, "which = 2")
    refused(wg(ctypes.byref(desc()), P(x), 0, P(x2), cout, c1 + 1, 0, P(dw), st), E_SHAPE, "c1_rows > C1")
    refused(wg(ctypes.byref(desc(c2=32)), P(x), 0, P(x2), cout, c1, 33, P(dw), st), E_SHAPE, "c2_rows > C2")
    refused(wg(ctypes.byref(desc(c1=12)), P(x), 0, P(x2), cout, 12, 0, P(dw), st), E_SHAPE, "wgrad C1 % 8")
    refused(wg(ctypes.byref(desc()), P(x), 0, P(x2), 60, c1, 0, P(dw), st), E_SHAPE, "dz_channels % 8 / < cout")
    refused(wg(ctypes.byref(desc()), P(x, 8), 0, P(x2), cout, c1, 0, P(dw), st), E_ALIGN, "wgrad misaligned x")
    refused(wg(ctypes.byref(desc()), P(x), 0, P(x2, 8), cout, c1, 0, P(dw), st), E_ALIGN, "wgrad misaligned dz")
    refused(lib.shdr_conv2d_wgrad_alltaps_f16(ctypes.byref(desc(stride=2, Ho=4, Wo=4)), P(x), 0, P(x2), cout, c1, 0, P(dw), st), E_SHAPE,
            "all-taps entry: a layer it does not take")
