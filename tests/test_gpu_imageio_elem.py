"""The image plumbing kernels (csrc/imageio.hip) against the float64 / index-arithmetic references of tests/imageio_ref.py, ELEMENT BY
ELEMENT.  tests/test_gpu_io.py compares resize_cubic with an fp32 restatement of the kernel under a
tensor-scale norm; here the reference is independent and no element can hide behind a larger one.

The C ABI is called through shdr._lib with every output between guard words.  Every family has one case with more work items than
one launch has threads (shdr::stream_grid: 2048 blocks x 256), so each grid-stride loop runs a second trip.  The inputs live in
imageio_ref.py; tests/test_imageio_ref.py shows on the CPU that a kernel with a wrong border, tap, coefficient, axis, coordinate rule,
reflection or rotation would fail AT THESE INPUTS.

resize_cubic, exact family: small integers and power-of-two ratios make every weight (a multiple of 2^-8 at worst), product and
partial sum exactly representable, so the result is the same in any order and with or without fused multiply-adds, and whole-tensor
equality of BIT PATTERNS is asked for.  The precondition -- the fp32 restatement equals the float64 reference in bits -- is asserted
before the launch.

resize_cubic, general ratios: |got - ref| <= A u S + B u T per element, u = 2^-24, S = sum |cy_i| |cx_j| |x_ij| and T = sum |x_ij| over
the element's 16 taps.  Derivation (nothing in it is fitted to a run):
  * The coordinate contributes nothing: t = f - floor(f) is the same fp32 number on both sides (imageio_ref.py).
  * Weight polynomials, fp32, each rounding at most half an ulp of its result, carried to the end by the factors that follow it
    (p = t + 1 < 2; intermediates reach 8 |A| = 6):
      c0 = ((A p - 5A) p + 8A) p - 4A: p itself u (times |dc0/dp| <= 0.75), A p u (times p^2 < 4), + 3.75 2u (times 4), times p 4u
           (times 2), - 6 2u (times 2), times p 2u, + 3 u/8: E0 <= 0.75 + 4 + 8 + 8 + 4 + 2 + 0.125 < 27 u
      c1 = ((A + 2) t - (A + 3)) t t + 1: u, 2u, u, u/2, u/2, later factors t <= 1: E1 <= 5 u
      c2 = the same in 1 - t, which may round by u/2 (times |dc2/ds| <= 1.35): E2 <= 5.7 u
      c3 = 1 - c0 - c1 - c2: E0 + E1 + E2 and three more roundings u, u, u/8: E3 <= 39.8 u =: E
    (tests/test_imageio_ref.py checks E0..E3 at 2^20 values of t.)  The weights themselves are at most 1, so the product of a row and
    a column weight is off by at most E (|cy_i| + |cx_j|) + E^2 <= 2E: over the 16 taps, 2 E T.  B = 82 >= 2 * 39.8 and the E^2 term.
  * 16 products and 15 sums: a tap passes through 2 products and at most 6 sums (the first sum of each row and of the column adds to
    zero), 8 roundings of relative size u on terms whose absolute values sum to S (+ 2 E T): A = 9 >= 8 / (1 - 8u) with room for the
    cross term 8u * 2E T and the float64 reference's own 1e-16.
A fused multiply-add drops a rounding and never adds one, so the bound holds however the compiler contracts the sums.

rgbe_encode is compared with oracle.imageio.rgbe_encode in bytes.  Radiances from 2^127 upward and non-finite values are out of
scope: the exponent byte e + 128 wraps there exactly as in Ward's code, and no test pins what that wrap should give."""
import numpy as np
import pytest
import torch

import imageio_ref as R
from oracle import imageio as O
from test_gpu_wgrad_f32_exact import P, guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def out_f32(numel):
    buf, view = guarded(numel)
    return buf, view, view.view(torch.float32)


def fetch(view_f32, shape):
    torch.cuda.synchronize()
    return view_f32.cpu().numpy().reshape(shape)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    view = np.uint32 if got.dtype == np.float32 else got.dtype
    bad = got.view(view) != want.view(view)
    if bad.any():
        i = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.size, i, got[i].item(), want[i].item()))


def run_resize(lib, x, out_hw, what):
    n, h, w, c = x.shape
    ho, wo = out_hw
    numel = n * ho * wo * c
    buf, view, y = out_f32(numel)
    xd = dev(x)
    assert lib.shdr_resize_cubic_f32(P(xd), P(y), n, h, w, c, ho, wo, None) == 0, what
    got = fetch(y, (n, ho, wo, c))
    guards_intact(buf, numel, what)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# resize_cubic
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CUBIC_EXACT, ids=R.case_id)
def test_resize_cubic_exact(lib, case):
    h, w, ho, wo, _ = case
    for n in (1, 2):
        for c in (1, 3, 4):
            what = "resize_cubic %s N=%d C=%d" % (R.case_id(case), n, c)
            x = R.cubic_exact_input(case, n, c)
            want, _, _ = R.cubic(x, (ho, wo))
            assert np.array_equal(O.resize_cubic(x, (ho, wo)).astype(np.float64), want), what + ": precondition (exact in fp32)"
            same_bits(run_resize(lib, x, (ho, wo), what), want.astype(np.float32), what)


@pytest.mark.parametrize("case", R.CUBIC_GENERAL, ids=R.case_id)
def test_resize_cubic_per_element(lib, case):
    n, h, w, c, ho, wo = case
    what = "resize_cubic " + R.case_id(case)
    x = R.cubic_general_input(case)
    want, S, T = R.cubic(x, (ho, wo))
    tol = R.cubic_tol(S, T)
    got = run_resize(lib, x, (ho, wo), what)
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / np.maximum(tol, 1e-300)
    i = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    print("%s: worst err / tol = %.3g at %s (err = %.1f u S, S = %.3g)" % (what, ratio[i], i, err[i] / (R.U * S[i]), S[i]))
    assert np.all(err <= tol), "%s: %d elements beyond the tolerance; worst at %s: got %r, want %r, err / tol = %.3g" % (
        what, int((err > tol).sum()), i, float(got[i]), float(want[i]), float(ratio[i]))


# ---------------------------------------------------------------------------------------------------------------------------------
# u8_to_unit, pad_symmetric, flip_rot90, rgbe_encode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 255, 256, 257, R.LAUNCH_THREADS + 257])
def test_u8_to_unit_exact(lib, npix):
    u8 = R.u8_pixels(npix)
    xd = dev(u8)
    for reverse in (0, 1):
        what = "u8_to_unit npix=%d reverse=%d" % (npix, reverse)
        buf, view, y = out_f32(3 * npix)
        assert lib.shdr_u8_to_unit_f32(P(xd), P(y), npix, reverse, None) == 0, what
        same_bits(fetch(y, (npix, 3)), R.u8_to_unit(u8, bool(reverse)), what)
        guards_intact(buf, 3 * npix, what)


def test_u8_to_unit_every_value_in_every_channel(shdr):
    u8 = R.u8_pixels(256).reshape(16, 16, 3)
    for reverse in (False, True):
        same_bits(shdr._ops.u8_to_unit(dev(u8), reverse).cpu().numpy(), R.u8_to_unit(u8, reverse), "u8_to_unit wrapper")


@pytest.mark.parametrize("case", R.PAD_CASES, ids=R.case_id)
def test_pad_symmetric_exact(lib, case):
    n, h, w, c, pad = case
    what = "pad_symmetric " + R.case_id(case)
    x = R.pad_input(case)
    want = R.pad_symmetric(x, pad)
    buf, view, y = out_f32(want.size)
    xd = dev(x)
    assert lib.shdr_pad_symmetric_f32(P(xd), P(y), n, h, w, c, pad, None) == 0, what
    same_bits(fetch(y, want.shape), want, what)
    guards_intact(buf, want.size, what)


@pytest.mark.parametrize("case", R.FLIP_CASES, ids=R.case_id)
def test_flip_rot90_exact(lib, case):
    s, c, divisor = case
    what = "flip_rot90 " + R.case_id(case)
    x, flip, k = R.flip_input(case)
    want = R.flip_rot90(x, flip, k, divisor)
    buf, view, y = out_f32(x.size)
    xd, fd, kd = dev(x), dev(flip), dev(k)
    assert lib.shdr_flip_rot90_f32(P(xd), P(y), P(fd), P(kd), x.shape[0], s, c, divisor, None) == 0, what
    same_bits(fetch(y, x.shape), want, what)
    guards_intact(buf, x.size, what)


@pytest.mark.parametrize("npix", [1, R.LAUNCH_THREADS + 3])
def test_rgbe_encode_bytes(lib, npix):
    x = R.rgbe_input(npix)
    xd = dev(x)
    for reverse in (0, 1):
        what = "rgbe_encode npix=%d reverse=%d" % (npix, reverse)
        buf, view = guarded(npix)                 # one 32-bit word per RGBE pixel
        assert lib.shdr_rgbe_encode_f32(P(xd), P(view), npix, reverse, None) == 0, what
        torch.cuda.synchronize()
        got = view.cpu().numpy().view(np.uint8).reshape(npix, 4)
        same_bits(got, O.rgbe_encode(x[:, ::-1] if reverse else x), what)
        guards_intact(buf, npix, what)
        if npix > 1 and not reverse:
            px, expect = R.rgbe_pixels()
            for row, ch, byte in expect:          # the truncating cast: j at j 2^(e-8), j - 1 one fp32 step below
                assert got[row, ch] == byte, (what, row, ch, byte, px[row].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: the code comes back and the output stays as it was
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(lib):
    x = dev(np.ones(4 * 6 * 6 * 3, dtype=np.float32))
    u8 = dev(np.ones(64 * 3, dtype=np.uint8))
    i32 = dev(np.zeros(4, dtype=np.int32))
    buf, view, y = out_f32(4096)
    calls = {
        "u8_to_unit null x": (E_NULL, lambda: lib.shdr_u8_to_unit_f32(None, P(y), 64, 0, None)),
        "u8_to_unit npix 0": (E_SHAPE, lambda: lib.shdr_u8_to_unit_f32(P(u8), P(y), 0, 0, None)),
        "u8_to_unit npix < 0": (E_SHAPE, lambda: lib.shdr_u8_to_unit_f32(P(u8), P(y), -5, 0, None)),
        "resize_cubic null x": (E_NULL, lambda: lib.shdr_resize_cubic_f32(None, P(y), 1, 6, 6, 3, 8, 8, None)),
        "pad_symmetric null x": (E_NULL, lambda: lib.shdr_pad_symmetric_f32(None, P(y), 1, 6, 6, 3, 2, None)),
        "pad_symmetric pad > H": (E_SHAPE, lambda: lib.shdr_pad_symmetric_f32(P(x), P(y), 1, 4, 9, 3, 5, None)),
        "pad_symmetric pad > W": (E_SHAPE, lambda: lib.shdr_pad_symmetric_f32(P(x), P(y), 1, 9, 4, 3, 5, None)),
        "pad_symmetric pad < 0": (E_SHAPE, lambda: lib.shdr_pad_symmetric_f32(P(x), P(y), 1, 6, 6, 3, -1, None)),
        "rgbe_encode null x": (E_NULL, lambda: lib.shdr_rgbe_encode_f32(None, P(y), 64, 0, None)),
        "rgbe_encode npix 0": (E_SHAPE, lambda: lib.shdr_rgbe_encode_f32(P(x), P(y), 0, 0, None)),
        "flip_rot90 null x": (E_NULL, lambda: lib.shdr_flip_rot90_f32(None, P(y), P(i32), P(i32), 4, 6, 3, 1.0, None)),
        "flip_rot90 null flip": (E_NULL, lambda: lib.shdr_flip_rot90_f32(P(x), P(y), None, P(i32), 4, 6, 3, 1.0, None)),
        "flip_rot90 null rot": (E_NULL, lambda: lib.shdr_flip_rot90_f32(P(x), P(y), P(i32), None, 4, 6, 3, 1.0, None)),
        "flip_rot90 divisor 0": (E_SHAPE, lambda: lib.shdr_flip_rot90_f32(P(x), P(y), P(i32), P(i32), 4, 6, 3, 0.0, None)),
        "flip_rot90 divisor -0": (E_SHAPE, lambda: lib.shdr_flip_rot90_f32(P(x), P(y), P(i32), P(i32), 4, 6, 3, -0.0, None)),
    }
    for off in (1, 2, 3):
        calls["rgbe_encode y misaligned by %d" % off] = (E_ALIGN, lambda off=off: lib.shdr_rgbe_encode_f32(P(x), P(y, off), 64, 0, None))
    for i, nm in enumerate(("N", "H", "W", "C", "Ho", "Wo")):
        for bad in (0, -1):
            dims = [1, 6, 6, 3, 8, 8]
            dims[i] = bad
            calls["resize_cubic %s = %d" % (nm, bad)] = (E_SHAPE, lambda d=dims: lib.shdr_resize_cubic_f32(P(x), P(y), *d, None))
    for i, nm in enumerate(("N", "H", "W", "C")):
        dims = [1, 6, 6, 3]
        dims[i] = 0
        calls["pad_symmetric %s = 0" % nm] = (E_SHAPE, lambda d=dims: lib.shdr_pad_symmetric_f32(P(x), P(y), *d, 1, None))
    for i, nm in enumerate(("N", "side", "C")):
        dims = [4, 6, 3]
        dims[i] = 0
        calls["flip_rot90 %s = 0" % nm] = (E_SHAPE, lambda d=dims: lib.shdr_flip_rot90_f32(P(x), P(y), P(i32), P(i32), *d, 1.0, None))
    for what, (code, call) in calls.items():
        assert call() == code, what
        untouched(buf, what)
    for what, call in {"u8_to_unit": lambda: lib.shdr_u8_to_unit_f32(P(u8), None, 64, 0, None),
                       "resize_cubic": lambda: lib.shdr_resize_cubic_f32(P(x), None, 1, 6, 6, 3, 8, 8, None),
                       "pad_symmetric": lambda: lib.shdr_pad_symmetric_f32(P(x), None, 1, 6, 6, 3, 2, None),
                       "rgbe_encode": lambda: lib.shdr_rgbe_encode_f32(P(x), None, 64, 0, None),
                       "flip_rot90": lambda: lib.shdr_flip_rot90_f32(P(x), None, P(i32), P(i32), 4, 6, 3, 1.0, None)}.items():
        assert call() == E_NULL, what + " null y"
