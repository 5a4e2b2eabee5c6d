"""The fp32 weight-gradient kernels (csrc/wgrad.hip, wgrad_winograd.hip, wgrad_x3.hip) against the float64 reference of
tests/conv_ref.py, EXACTLY and element by element.

Inputs are small integers: x, dz in [-2, 2]; the second source holds multiples of 1 / x2_scale with x2_scale a power of two (0.5 or
2^-8), so that the scaled source is again in [-2, 2].  Every product is then an integer and every fp32 partial sum of at most 2^22
of them is exact in ANY order: split-K slices whose size depends on the CU count, fp32 atomics, the MFMA accumulation order and the
fp16 / bf16 operand rounding of the PREC = 1 / 2 forms cannot excuse a difference.  In the Winograd domain B^T d B and A dY A^T are
integers and G holds halves: every value is a multiple of 1/4.  The split-operand kernel gets one operand of the form
(k + j 2^-11) 2^-T, which its split pass takes apart into exactly (k, j), and one integer operand whose low plane is empty: the dropped
Xl Zl term is zero, each cross term is tested on its own, and the epilogue's hi + lo / 2048 is exact below 2048 pixels.  Each test
asserts its precondition (operand forms, and the sum of absolute terms in units of the smallest term below 2^24) before it launches.

Every comparison is whole-tensor equality of BIT PATTERNS.  dw is ACCUMULATED (`dw +=`, include/shdr.h), so each family runs into
zeros and into integers, and the elements the ABI must not touch -- the rows of the other source, everything outside
[ci_off, ci_off + Cx) -- hold finite sentinels: -12345 at even offsets and -0.0 at odd ones.  A NaN would swallow a stray atomic add;
-12345 shows any stray non-zero addend; -0.0 shows even a stray `+= 0.0f` (the sum is +0.0).  Buffers sit between guard words.

The C ABI is called through shdr._lib: the Python wrapper pads channel counts, never reaches the direct kernel and picks the family."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as C

pytestmark = pytest.mark.gpu

GUARD = 64
SENT32 = 0x7FC5A5A5
SENT16 = 0x7E5A
FINITE = -12345.0
E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5
AUTO, MFMA, DIRECT, MFMA_F16, MFMA_BF16, AUTO_F16 = 0, 1, 2, 4, 5, 6
S8 = 2.0 ** -8
LIMIT = 2 ** 24


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


# ---------------------------------------------------------------------------------------------------------------------------------
# operands, buffers, assertions
# ---------------------------------------------------------------------------------------------------------------------------------
def ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def f32(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a), "operand not exact in fp32"
    return torch.from_numpy(a.astype(np.float32)).cuda()


def P(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off)


def guarded(numel, dtype=torch.int32):
    """(whole buffer, view of `numel` elements between two GUARDs), filled with a NaN pattern; the view is 16-byte aligned"""
    buf = torch.full((numel + 2 * GUARD,), SENT16 if dtype == torch.int16 else SENT32, device="cuda", dtype=dtype)
    view = buf[GUARD:GUARD + numel]
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf, numel, what):
    torch.cuda.synchronize()
    sent = SENT16 if buf.dtype == torch.int16 else SENT32
    assert bool((buf[:GUARD] == sent).all()), what + ": words BEFORE the tensor were written"
    assert bool((buf[GUARD + numel:] == sent).all()), what + ": words PAST the tensor were written"


def untouched(buf, what):
    torch.cuda.synchronize()
    assert bool((buf == (SENT16 if buf.dtype == torch.int16 else SENT32)).all()), what + ": a refused call wrote its output"


def forbidden(shape):
    """what the elements hold that the call must not touch: -12345 at even offsets, -0.0 at odd ones"""
    a = np.full(shape, FINITE, dtype=np.float32)
    a.reshape(-1)[1::2] = -0.0
    return a


def same(got, want, what, tile=None):
    """strict equality of bit patterns, so that a -0.0 that became +0.0 shows.  A difference names the first differing index, its tap
    and tile (dw [kh, kw, ci, co] with `tile` = (CI_T, CO_T)) and got / want there."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    bad = got.view(bits) != want.view(bits)
    if bad.any():
        i = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        where = ""
        if tile is not None and len(i) == 4:
            where = ", tap (%d, %d), tile (%d, %d) of %s" % (i[0], i[1], i[2] // tile[0], i[3] // tile[1], tuple(tile))
        raise AssertionError("%s: %d of %d elements differ; first at %s%s: got %r, want %r"
                             % (what, int(bad.sum()), bad.size, i, where, float(got[i]), float(want[i])))


def small_ints(a, scale, what):
    q = np.asarray(a, dtype=np.float64) * scale
    assert np.array_equal(q, np.rint(q)) and float(np.abs(q).max(initial=0.0)) <= 2, what + ": operand is not an integer in [-2, 2]"


def precondition(sources, dz, npix, base, what):
    """x (times its scale) and dz are integers in [-2, 2]: at most `npix` products of magnitude <= 4 meet in one element of dw, all in
    units of one; with the caller's integers the sum of absolute terms stays below 2^24"""
    for a, s in sources:
        small_ints(a, s, what)
    small_ints(dz, 1.0, what)
    assert 4 * npix + float(np.abs(base).max(initial=0.0)) < LIMIT, what


def desc_of(K, x_shape, c2, k, cols, stride, x2s=1.0, cout=None, algo=AUTO):
    """descriptor of a 'SAME' layer whose gradient has `cols` columns (cout_valid); Cout = `cout` (>= cols) is the padded width"""
    khw = (k, k) if isinstance(k, int) else tuple(k)
    d = K._conv_desc(tuple(x_shape), khw + (x_shape[3] + c2, cout or cols), stride, c2, x2s, cols)
    d.algo = algo
    return d


def base_of(shape, accumulate, seed):
    if not accumulate:
        return np.zeros(shape, dtype=np.float32)
    return np.random.default_rng(seed).integers(-50, 51, size=shape).astype(np.float32)


def operands(seed, n, h, w, c1, c2, cz, k, stride, x2s):
    rng = np.random.default_rng(seed)
    x = ints(rng, (n, h, w, c1), -2, 2)
    x2 = ints(rng, (n, h, w, c2), -2, 2) / x2s if c2 else None
    dz = ints(rng, (n, -(-h // stride), -(-w // stride), cz), -2, 2)
    return x, x2, dz


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_conv2d_wgrad_f32: wgrad_mfma_kernel, wgrad_alltaps_kernel, wgrad_direct_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def run_wgrad(K, lib, x, x2, dz, k, stride, x2s=1.0, algo=AUTO, cout=None, accumulate=False, what="wgrad", tile=(16, 16), x_off=0):
    """dw [k, k, C1 + C2, cols] between guards.  Source 0 runs with the rows of source 1 holding the sentinels, then source 1 with
    the rows of source 0 holding them: each call is compared as a whole tensor."""
    c1, c2 = x.shape[3], 0 if x2 is None else x2.shape[3]
    cols = dz.shape[3]
    ref = C.wgrad(x, x2, dz, (k, k, c1 + c2, cols), stride, x2s, None)
    npix = dz.shape[0] * dz.shape[1] * dz.shape[2]
    base = base_of(ref.shape, accumulate, c1 * 7 + cols)
    precondition([(x, 1.0)] + ([(x2, x2s)] if c2 else []), dz, npix, base, what)
    assert np.array_equal(ref, np.rint(ref))
    buf, v = guarded(ref.size)
    dw = v.view(torch.float32).view(ref.shape)
    d = desc_of(K, x.shape, c2, k, cols, stride, x2s, cout, algo)
    assert tuple(dz.shape[:3]) == (x.shape[0], d.Ho, d.Wo)
    dzd = f32(dz)
    for which, src, r0, r1 in ((0, x, 0, c1),) + (((1, x2, c1, c1 + c2),) if c2 else ()):
        init = forbidden(ref.shape)
        init[:, :, r0:r1] = base[:, :, r0:r1]
        want = init.copy()
        want[:, :, r0:r1] += ref[:, :, r0:r1].astype(np.float32)
        dw.copy_(torch.from_numpy(init))
        if x_off:                                                        # the same values at an address that is not 16-byte aligned
            store = torch.zeros((src.size + 4,), device="cuda", dtype=torch.float32)
            store[x_off // 4:x_off // 4 + src.size].copy_(f32(src).view(-1))
            xd, ptr = store, P(store, x_off)
        else:
            xd = f32(src)
            ptr = P(xd)
        rc = lib.shdr_conv2d_wgrad_f32(ctypes.byref(d), ptr, which, P(dzd), P(dw), K._stream())
        assert rc == 0, (what, rc, lib.shdr_last_error())
        guards_intact(buf, ref.size, what)
        same(dw.cpu().numpy(), want, "%s (source %d; the other rows untouched)" % (what, which), tile)
    return d


# wgrad_mfma_kernel<BMc, BNc, WM, WN, PREC> (SHDR_NO_ALLTAPS set).  Dispatch (shdr_conv2d_wgrad_f32): BMc by Cx -- % 128 -> 128; % 64 -> 64;
# % 96 with cols % 32 == 0 and SHDR_NO_WGRAD96 unset -> 96; % 32 -> 32; else 16 -- and BNc by cols (= cout_valid) -- % 128 -> 128;
# % 64 -> 64; % 32 -> 32; else 16.  <96, 16> does not exist: 96 channels with 16 columns run on three 32-row tiles.  A slice is a
# multiple of 32 pixels and at least 1024 (SHDR_WGRAD_LEGACY_GRID: 2048).
# Every (tile pair, PREC) form gets a RAGGED pixel count -- 1, 31, 33, 65 or 510 (a batch of two odd images): none is a multiple of the
# 32-pixel chunk.  The size moves on by one per form and once more per PREC, so a tile pair meets three sizes and every size meets every
# BMc and BNc.  288 pixels (2 x 9 x 16: nine full chunks, the control without a ragged chunk) come as extra cases below, one per PREC.
RAGGED = [(1, 1, 1), (1, 1, 31), (1, 3, 11), (1, 5, 13), (2, 15, 17)]
MFMA_CASES = []
# id, n, h, w, c1, c2, cols, k, stride, x2s, (BMc, BNc), opts
for _p, (_prec, _algo) in enumerate((("f32", MFMA), ("f16", MFMA_F16), ("bf16", MFMA_BF16))):
    for _cx, _bm in ((16, 16), (32, 32), (64, 64), (96, 96), (128, 128)):
        for _cz, _bn in ((16, 16), (32, 32), (64, 64), (128, 128)):
            _n, _h, _w = RAGGED[(len(MFMA_CASES) + _p) % len(RAGGED)]
            assert (_n * _h * _w) % 32 != 0
            _t = (32, 16) if (_cx, _cz) == (96, 16) else (_bm, _bn)
            MFMA_CASES.append(("tile_%dx%d_%s_%dx%dx%d" % (_t[0], _t[1], _prec, _n, _h, _w), _n, _h, _w, _cx, 0, _cz, 3, 1, 1.0, _t,
                               {"algo": _algo}))
MFMA_CASES += [
    ("auto_algo_32x32", 2, 9, 16, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),
    ("full_chunks_288_64x64_f32", 2, 9, 16, 64, 0, 64, 3, 1, 1.0, (64, 64), {"algo": MFMA}),
    ("full_chunks_288_96x128_f16", 2, 9, 16, 96, 0, 128, 3, 1, 1.0, (96, 128), {"algo": MFMA_F16}),
    ("full_chunks_288_128x128_bf16", 2, 9, 16, 128, 0, 128, 3, 1, 1.0, (128, 128), {"algo": MFMA_BF16}),
    ("no_wgrad96_cx96_on_32_tiles", 2, 15, 17, 96, 0, 64, 3, 1, 1.0, (32, 64), {"env": "SHDR_NO_WGRAD96"}),
    ("cx48_three_16_tiles", 1, 5, 13, 48, 0, 32, 3, 1, 1.0, (16, 32), {}),
    ("cx160_five_32_tiles", 1, 3, 11, 160, 0, 16, 3, 1, 1.0, (32, 16), {}),
    ("cols48_three_16_tiles", 1, 5, 13, 32, 0, 48, 3, 1, 1.0, (32, 16), {}),
    ("cols192_three_64_tiles", 1, 1, 31, 64, 0, 192, 3, 1, 1.0, (64, 64), {}),
    ("cx288_three_96_tiles", 1, 3, 11, 288, 0, 32, 1, 1, 1.0, (96, 32), {}),
    ("pixels_1025_past_a_slice", 1, 25, 41, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),
    ("pixels_2115_slices", 1, 47, 45, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),
    ("pixels_2115_slices_128x64_f16", 1, 47, 45, 128, 0, 64, 3, 1, 1.0, (128, 64), {"algo": MFMA_F16}),
    ("pixels_2115_slices_16x16_bf16", 1, 47, 45, 16, 0, 16, 3, 1, 1.0, (16, 16), {"algo": MFMA_BF16}),
    ("legacy_pixels_2049_past_a_slice", 1, 3, 683, 32, 0, 32, 3, 1, 1.0, (32, 32), {"env": "SHDR_WGRAD_LEGACY_GRID"}),
    ("legacy_pixels_4200_slices", 1, 56, 75, 64, 0, 32, 3, 1, 1.0, (64, 32), {"env": "SHDR_WGRAD_LEGACY_GRID"}),
    ("legacy_pixels_33", 1, 3, 11, 16, 0, 64, 3, 1, 1.0, (16, 64), {"env": "SHDR_WGRAD_LEGACY_GRID"}),
    ("k1", 2, 15, 17, 64, 0, 32, 1, 1, 1.0, (64, 32), {}),
    ("k5", 2, 9, 16, 32, 0, 64, 5, 1, 1.0, (32, 64), {}),
    ("k7", 1, 15, 17, 16, 0, 16, 7, 1, 1.0, (16, 16), {}),
    ("k7_f16", 1, 5, 13, 16, 0, 32, 7, 1, 1.0, (16, 32), {"algo": MFMA_F16}),
    ("s2_1x1_odd", 2, 15, 17, 64, 0, 128, 1, 2, 1.0, (64, 128), {}),
    ("s2_3x3_odd", 2, 15, 17, 32, 0, 64, 3, 2, 1.0, (32, 64), {}),
    ("s2_7x7_odd_stem_96", 2, 15, 17, 96, 0, 64, 7, 2, 1.0, (96, 64), {}),
    ("s2_3x3_odd_bf16", 2, 17, 15, 16, 0, 16, 3, 2, 1.0, (16, 16), {"algo": MFMA_BF16}),
    ("two_sources_32_32_scaled", 2, 17, 15, 32, 32, 64, 3, 1, S8, (32, 64), {}),
    ("two_sources_64_16_half", 1, 5, 13, 64, 16, 16, 3, 1, 0.5, (64, 16), {}),
    ("two_sources_96_32_scaled_f16", 1, 3, 11, 96, 32, 32, 3, 1, S8, (96, 32), {"algo": MFMA_F16}),
    ("two_sources_16_128_scaled_bf16", 1, 1, 31, 16, 128, 32, 1, 1, S8, (16, 32), {"algo": MFMA_BF16}),
    ("cout_valid_16_of_32", 2, 9, 16, 32, 0, 16, 3, 1, 1.0, (32, 16), {"cout": 32}),
    ("cout_valid_16_of_32_two_sources", 1, 5, 13, 16, 16, 16, 3, 1, S8, (16, 16), {"cout": 32}),
    ("accumulate_64x32", 2, 15, 17, 64, 0, 32, 3, 1, 1.0, (64, 32), {"accumulate": True}),
    ("accumulate_two_sources_slices", 1, 47, 45, 32, 32, 16, 3, 1, S8, (32, 16), {"accumulate": True}),
    ("accumulate_f16", 1, 5, 13, 32, 0, 32, 3, 1, 1.0, (32, 32), {"accumulate": True, "algo": MFMA_F16}),
]


def run_case(K, lib, case, monkeypatch, algo=AUTO):
    name, n, h, w, c1, c2, cz, k, stride, x2s, tile, o = case
    if o.get("env"):
        monkeypatch.setenv(o["env"], "1")
    x, x2, dz = operands(len(name) * 41 + h * 3 + w, n, h, w, c1, c2, cz, k, stride, x2s)
    return run_wgrad(K, lib, x, x2, dz, k, stride, x2s, o.get("algo", algo), o.get("cout"), o.get("accumulate", False), name, tile,
                     o.get("x_off", 0))


@pytest.mark.parametrize("case", MFMA_CASES, ids=[c[0] for c in MFMA_CASES])
def test_mfma_kernel(K, lib, case, monkeypatch):
    monkeypatch.setenv("SHDR_NO_ALLTAPS", "1")
    run_case(K, lib, case, monkeypatch)


# wgrad_alltaps_kernel<KK, MT, NT>: stride 1, Cx and cols in {16, 32}, k 3 (all four), k 5 (Cx * cols <= 512: three), k 7 (16 -> 16): the
# eight triples of the predicate are the eight instantiations.  One block takes `slice` row segments of 32 pixels; the grid holds at most
# 1024 blocks, so only more than 1024 segments give a block a second unit (the double-buffered loop).
ALLTAPS_SIZES = [(1, 1, 1), (1, 5, 70), (1, 33, 50), (2, 9, 40)]
ALLTAPS = []
for _k, _pairs in ((3, ((16, 16), (16, 32), (32, 16), (32, 32))), (5, ((16, 16), (16, 32), (32, 16))), (7, ((16, 16),))):
    for _cx, _cz in _pairs:
        for _n, _h, _w in (ALLTAPS_SIZES[len(ALLTAPS) % 4], ALLTAPS_SIZES[(len(ALLTAPS) + 2) % 4]):
            ALLTAPS.append(("alltaps_k%d_%d_%d_%dx%dx%d" % (_k, _cx, _cz, _n, _h, _w), _n, _h, _w, _cx, 0, _cz, _k, 1, 1.0, (_cx, _cz), {}))
ALLTAPS += [
    ("alltaps_k7_33x50", 1, 33, 50, 16, 0, 16, 7, 1, 1.0, (16, 16), {}),
    ("alltaps_k5_32_16_batch2", 2, 9, 40, 32, 0, 16, 5, 1, 1.0, (32, 16), {}),
    ("alltaps_two_units_per_block_k3_32_32", 1, 70, 513, 32, 0, 32, 3, 1, 1.0, (32, 32), {}),          # 70 * 17 = 1190 segments
    ("alltaps_two_units_per_block_k5_16_16", 2, 37, 449, 16, 0, 16, 5, 1, 1.0, (16, 16), {}),          # 2 * 37 * 15 = 1110
    ("alltaps_two_sources_32_32_scaled", 1, 33, 50, 32, 32, 32, 3, 1, S8, (32, 32), {}),
    ("alltaps_two_sources_16_32_half_k5", 1, 5, 70, 16, 32, 16, 5, 1, 0.5, (16, 16), {}),
    ("alltaps_accumulate_k7", 2, 9, 40, 16, 0, 16, 7, 1, 1.0, (16, 16), {"accumulate": True}),
    ("alltaps_accumulate_two_sources", 1, 33, 50, 32, 16, 32, 3, 1, S8, (32, 32), {"accumulate": True}),
    ("alltaps_auto_f16_stays_exact_fp32", 1, 5, 70, 32, 0, 32, 3, 1, 1.0, (32, 32), {"algo": AUTO_F16}),
]


@pytest.mark.parametrize("case", ALLTAPS, ids=[c[0] for c in ALLTAPS])
def test_all_taps_kernel(K, lib, case, monkeypatch):
    run_case(K, lib, case, monkeypatch)


def test_all_taps_declines_5x5_32_32_and_the_per_tap_kernel_answers(K, lib, monkeypatch):
    """Cx * cols = 1024 > 512: over the register budget of <5, 2, 2>; the layer runs on wgrad_mfma_kernel<32, 32>"""
    run_case(K, lib, ("alltaps_declined_k5_32_32", 1, 33, 50, 32, 0, 32, 5, 1, 1.0, (32, 32), {}), monkeypatch)


# wgrad_direct_kernel: channel counts off the 16 grid, SHDR_ALGO_DIRECT, or an operand that is not 16-byte aligned; 1024 pixels per block
DIRECT_CASES = [
    ("direct_3_3_pixels_1", 1, 1, 1, 3, 0, 3, 3, 1, 1.0, (3, 3), {}),
    ("direct_3_3_pixels_1024", 1, 32, 32, 3, 0, 3, 3, 1, 1.0, (3, 3), {}),
    ("direct_4_16_pixels_1025", 1, 25, 41, 4, 0, 16, 3, 1, 1.0, (4, 16), {}),
    ("direct_16_3_of_16_pixels_2049", 1, 3, 683, 16, 0, 3, 3, 1, 1.0, (16, 3), {"cout": 16}),
    ("direct_algo_on_32_32", 2, 15, 17, 32, 0, 32, 3, 1, 1.0, (32, 32), {"algo": DIRECT}),
    ("direct_x_offset_4_bytes_32_32", 2, 9, 16, 32, 0, 32, 3, 1, 1.0, (32, 32), {"x_off": 4}),
    ("direct_two_sources_3_3_scaled", 2, 15, 17, 3, 3, 3, 1, 1, S8, (3, 3), {}),
    ("direct_two_sources_4_5_half_k5_s2", 1, 15, 17, 4, 5, 7, 5, 2, 0.5, (4, 7), {}),
    ("direct_accumulate_two_sources", 1, 25, 41, 3, 4, 3, 3, 1, S8, (3, 3), {"accumulate": True}),
    ("direct_algo_two_sources_16_16", 1, 5, 13, 16, 16, 16, 3, 1, S8, (16, 16), {"algo": DIRECT, "accumulate": True}),
]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=[c[0] for c in DIRECT_CASES])
def test_direct_kernel(K, lib, case, monkeypatch):
    run_case(K, lib, case, monkeypatch)


@pytest.mark.parametrize("algo", [MFMA, MFMA_F16, MFMA_BF16])
def test_forced_mfma_on_a_layer_it_cannot_take_is_refused(K, lib, algo):
    x = torch.zeros((2 * 9 * 16 * 32 + 4,), device="cuda")
    dz = torch.zeros((2 * 9 * 16 * 32,), device="cuda")
    buf, dw = guarded(9 * 32 * 32)
    for what, c1, cols, off in (("3 -> 3", 3, 3, 0), ("16 -> 3", 16, 3, 0), ("4 -> 16", 4, 16, 0), ("x off the 16-byte grid", 32, 32, 4)):
        d = desc_of(K, (2, 9, 16, c1), 0, 3, cols, 1, algo=algo)
        assert lib.shdr_conv2d_wgrad_f32(ctypes.byref(d), P(x, off), 0, P(dz), P(dw), K._stream()) == E_ALIGN, what
        untouched(buf, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_conv2d_wgrad_winograd_f32: wgrad_winograd_kernel<2> + winograd_dw_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def run_winograd(K, lib, n, h, w, c1, c2, cout, x2s, accumulate, what, seed):
    x, x2, dz = operands(seed, n, h, w, c1, c2, cout, 3, 1, x2s)
    ct = c1 + c2
    ref = C.wgrad(x, x2, dz, (3, 3, ct, cout), 1, x2s, None)
    base = base_of(ref.shape, accumulate, seed)
    # |B^T d B| <= 8 and |A dY A^T| <= 8 are integers: a dU element sums `tiles` products of magnitude <= 64; dW = G^T dU G has 16
    # terms with |G| <= 1 and is a multiple of scale / 4
    tiles = n * ((h + 1) // 2) * ((w + 1) // 2)
    for src, s in ((x, 1.0),) + (((x2, x2s),) if c2 else ()):
        small_ints(src, s, what)
        assert 4 * 16 * 64 * tiles + 4 * float(np.abs(base).max(initial=0.0)) / min(s, 1.0) < LIMIT, what
    small_ints(dz, 1.0, what)
    buf, v = guarded(ref.size)
    dw = v.view(torch.float32).view(ref.shape)
    dzd = f32(dz)
    for src, cx, off, s in ((x, c1, 0, 1.0),) + (((x2, c2, c1, x2s),) if c2 else ()):
        init = forbidden(ref.shape)
        init[:, :, off:off + cx] = base[:, :, off:off + cx]
        want = init.copy()
        want[:, :, off:off + cx] += ref[:, :, off:off + cx].astype(np.float32)
        dw.copy_(torch.from_numpy(init))
        dubuf, du = guarded(16 * cx * cout)
        du.view(torch.float32).fill_(FINITE)                            # the call zeroes its scratch
        xd = f32(src)
        rc = lib.shdr_conv2d_wgrad_winograd_f32(P(xd), P(dzd), P(du), P(dw), n, h, w, cx, cout, ct, off, s, K._stream())
        assert rc == 0, (what, rc, lib.shdr_last_error())
        guards_intact(buf, ref.size, what)
        guards_intact(dubuf, 16 * cx * cout, what + " (dU scratch)")
        same(dw.cpu().numpy(), want, "%s (rows [%d, %d); all others untouched)" % (what, off, off + cx), (32, 64))


# one block = 32 input channels x 64 output channels; a unit = 2 rows x 16 columns of output pixels; >= 32 units per slice
WINO_SIZES = [(1, 1, 1), (1, 2, 2), (1, 3, 17), (1, 13, 19), (1, 16, 32), (1, 33, 50), (3, 13, 19), (3, 33, 50), (2, 16, 32)]
WINO = []
for _cx in (32, 64, 96):
    for _cout in (64, 128, 192):
        _n, _h, _w = WINO_SIZES[len(WINO)]
        WINO.append(("wino_%d_%d_%dx%dx%d" % (_cx, _cout, _n, _h, _w), _n, _h, _w, _cx, 0, _cout, 1.0, False))
WINO += [
    ("wino_32_64_slices_3x33x50", 3, 33, 50, 32, 0, 64, 1.0, False),                    # 3 * 17 * 4 = 204 units: seven slices
    ("wino_64_64_1x1", 1, 1, 1, 64, 0, 64, 1.0, False),
    ("wino_32_64_2x2", 1, 2, 2, 32, 0, 64, 1.0, False),
    ("wino_64_128_3x17", 1, 3, 17, 64, 0, 128, 1.0, False),
    ("wino_32_64_16x32", 1, 16, 32, 32, 0, 64, 1.0, False),
    ("wino_two_sources_32_64_half", 1, 13, 19, 32, 64, 64, 0.5, False),                 # ci_off = 32, Ct = 96
    ("wino_two_sources_64_32_scaled_slices", 3, 33, 50, 64, 32, 64, S8, False),
    ("wino_accumulate", 3, 13, 19, 32, 0, 128, 1.0, True),
    ("wino_accumulate_two_sources_half", 1, 33, 50, 32, 32, 64, 0.5, True),
]


@pytest.mark.parametrize("case", WINO, ids=[c[0] for c in WINO])
def test_winograd_domain_kernels(K, lib, case):
    name, n, h, w, c1, c2, cout, x2s, acc = case
    run_winograd(K, lib, n, h, w, c1, c2, cout, x2s, acc, name, len(name) * 13 + h)


def test_winograd_domain_refusals(K, lib):
    x = torch.zeros((9 * 16 * 64 + 4,), device="cuda")
    dz = torch.zeros((9 * 16 * 192 + 4,), device="cuda")
    dubuf, du = guarded(16 * 64 * 192)
    buf, dw = guarded(9 * 128 * 192)
    call = lib.shdr_conv2d_wgrad_winograd_f32
    st = K._stream()
    for what, code, args in (
            ("Cx % 32", E_SHAPE, (P(x), P(dz), P(du), P(dw), 1, 9, 16, 48, 64, 48, 0, 1.0)),
            ("Cx 16", E_SHAPE, (P(x), P(dz), P(du), P(dw), 1, 9, 16, 16, 64, 16, 0, 1.0)),
            ("Cout % 64", E_SHAPE, (P(x), P(dz), P(du), P(dw), 1, 9, 16, 32, 96, 32, 0, 1.0)),
            ("x misaligned", E_ALIGN, (P(x, 4), P(dz), P(du), P(dw), 1, 9, 16, 32, 64, 32, 0, 1.0)),
            ("dz misaligned", E_ALIGN, (P(x), P(dz, 8), P(du), P(dw), 1, 9, 16, 32, 64, 32, 0, 1.0)),
            ("Ct < Cx", E_SHAPE, (P(x), P(dz), P(du), P(dw), 1, 9, 16, 64, 64, 32, 0, 1.0)),
            ("ci_off + Cx > Ct", E_SHAPE, (P(x), P(dz), P(du), P(dw), 1, 9, 16, 32, 64, 48, 32, 1.0)),
            ("negative ci_off", E_SHAPE, (P(x), P(dz), P(du), P(dw), 1, 9, 16, 32, 64, 64, -32, 1.0))):
        assert call(*args, st) == code, (what, lib.shdr_last_error())
        untouched(buf, what)
        untouched(dubuf, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_x3_split_planes_f32, bit-exact against conv_ref.split_planes
# ---------------------------------------------------------------------------------------------------------------------------------
def slot_of(bits_or_value):
    """a range slot: one device word holding the fp32 bound, or (an int) the given bit pattern"""
    if isinstance(bits_or_value, int):
        word = np.array([bits_or_value], dtype=np.uint32)
    else:
        word = np.array([bits_or_value], dtype=np.float32)
    return torch.from_numpy(word.view(np.int32)).cuda()


def slot_value(slot):
    return slot.cpu().numpy().view(np.float32)[0]


def scaled_values(n, seed):
    """values of the SCALED tensor, |v| < 2048: every fp16 binade from below the smallest denormal (2^-26) to 2^10 with random 24-bit
    mantissas, exact ties of the fp16 rounding (even and odd neighbours) and their fp32 neighbours, +0, -0, and both signs"""
    rng = np.random.default_rng(seed)
    b = (np.arange(n) % 37) - 26
    v = np.ldexp(1.0 + rng.integers(0, 2 ** 23, size=n) / 2.0 ** 23, b)
    kind = (np.arange(n) // 37) % 4
    q = rng.integers(1024, 2048, size=n).astype(np.float64)
    step = np.ldexp(1.0, np.maximum(b, -14) - 10)                         # fp16 spacing in the binade (denormals: 2^-24)
    tie = (np.where(b >= -14, q, q % 16) + 0.5) * step
    v = np.where(kind == 1, tie, v)
    v = np.where(kind == 2, tie * (1.0 + 2.0 ** -23), v)
    v = np.where(kind == 3, tie * (1.0 - 2.0 ** -24), v)
    v = v * rng.choice([-1.0, 1.0], size=n)
    v[5::97] = 0.0
    v[6::97] = -0.0
    return v


def run_split(K, lib, x, slot, what):
    """the planes are compared as fp16 bit patterns, signs of zeros included: conv_ref.split_planes models the +0 addend of the
    kernel's FMAs, which turns a -0 input into +0 while a negative value that underflows keeps its sign as -0"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.size
    hbuf, hi = guarded(n, torch.int16)
    lbuf, lo = guarded(n, torch.int16)
    xd = torch.from_numpy(x).cuda()
    rc = lib.shdr_x3_split_planes_f32(P(xd), n, P(slot), P(hi), P(lo), K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    guards_intact(hbuf, n, what + " (high plane)")
    guards_intact(lbuf, n, what + " (low plane)")
    want_hi, want_lo = (p.reshape(-1) for p in C.split_planes(x, slot_value(slot)))
    same(hi.cpu().numpy().view(np.float16), want_hi, what + " high plane")
    same(lo.cpu().numpy().view(np.float16), want_lo, what + " low plane")
    return hi, lo


SLOTS = [("two", 2.0), ("one", 1.0), ("below_one", float(np.nextafter(np.float32(1.0), np.float32(0.0)))), ("own_maximum", None),
         ("zero", 0.0), ("inf", float("inf")), ("nan_bits", 0x7FC5A5A5), ("sign_bit", -3.0), ("tiny_clamped", 2.0 ** -120),
         ("denormal_clamped", 1), ("largest_unclamped", 2.0 ** -115), ("huge", float(np.finfo(np.float32).max)), ("large", 6.0e4)]


@pytest.mark.parametrize("slot", SLOTS, ids=[s[0] for s in SLOTS])
def test_split_planes_slots(K, lib, slot):
    name, bound = slot
    v = scaled_values(2040, len(name))
    if bound is None:                                                    # the tensor's own maximum, not a power of two
        x = np.ldexp(v, -3).astype(np.float32)
        sl = slot_of(float(np.abs(x).max()))
    else:
        sl = slot_of(bound)
        x = np.ldexp(v, -C.range_exponent(slot_value(sl))).astype(np.float32)   # (rounded where that is denormal: it is the input)
    if name in ("tiny_clamped", "denormal_clamped"):
        assert C.range_exponent(slot_value(sl)) == 126 and (np.abs(x[x != 0]) < 2.0 ** -126).any(), "denormal fp32 inputs wanted"
    run_split(K, lib, x, sl, name)


@pytest.mark.parametrize("n", [8, 16, 2040, 8 * (2048 * 256 + 1)])
def test_split_planes_sizes(K, lib, n):
    """the last size is one 8-element item past the grid cap of shdr::stream_grid (2048 blocks of 256 threads)"""
    reps = -(-n // 4096)
    x = np.tile(np.ldexp(scaled_values(4096, 3), -9), reps)[:n]
    run_split(K, lib, x, slot_of(2.0), "n = %d" % n)


def test_split_planes_refusals(K, lib):
    x = torch.zeros((64,), device="cuda")
    hbuf, hi = guarded(64, torch.int16)
    lbuf, lo = guarded(64, torch.int16)
    sl = slot_of(2.0)
    st = K._stream()
    call = lib.shdr_x3_split_planes_f32
    for what, code, args in (("n % 8", E_ALIGN, (P(x), 12, P(sl), P(hi), P(lo))), ("n = 0", E_ALIGN, (P(x), 0, P(sl), P(hi), P(lo))),
                             ("n < 0", E_ALIGN, (P(x), -8, P(sl), P(hi), P(lo))), ("x misaligned", E_ALIGN, (P(x, 4), 8, P(sl), P(hi), P(lo))),
                             ("hi misaligned", E_ALIGN, (P(x), 8, P(sl), P(hi, 8), P(lo))), ("lo misaligned", E_ALIGN, (P(x), 8, P(sl), P(hi), P(lo, 2))),
                             ("null x", E_NULL, (None, 8, P(sl), P(hi), P(lo))), ("null slot", E_NULL, (P(x), 8, None, P(hi), P(lo))),
                             ("null hi", E_NULL, (P(x), 8, P(sl), None, P(lo))), ("null lo", E_NULL, (P(x), 8, P(sl), P(hi), None))):
        assert call(*args, st) == code, (what, lib.shdr_last_error())
        untouched(hbuf, what)
        untouched(lbuf, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_conv2d_wgrad_x3_f32: wgrad_x3_kernel<CI_T, CO_T>
# ---------------------------------------------------------------------------------------------------------------------------------
# (k, j) that the split pass takes apart exactly: fp16(k + j 2^-11) = k (ties go to the even mantissa of 1 and 2), the rest is j
FINE_PAIRS = np.array([(0, 0), (1, 0), (-1, 0), (1, 1), (-1, -1), (2, 0), (-2, 0), (2, 1), (2, 2), (2, -1), (-2, -1), (-2, -2), (-2, 1)],
                      dtype=np.float64)


def fine_operand(rng, shape, t):
    """((k + j 2^-11) 2^-t, k, j)"""
    kj = FINE_PAIRS[rng.integers(0, len(FINE_PAIRS), size=shape)]
    k, j = kj[..., 0], kj[..., 1]
    return np.ldexp(k + np.ldexp(j, -11), -t), k, j


def run_x3_source(K, lib, d, which, src, dz, x_bound, z_bound, fine, dw, buf, init, want, what, tile):
    """split both tensors on the device (checked bit for bit against the reference planes), then one call of the kernel"""
    xs, zs = slot_of(x_bound), slot_of(z_bound)
    xh, xl = run_split(K, lib, src, xs, what + " x")
    zh, zl = run_split(K, lib, dz, zs, what + " dz")
    dw.copy_(torch.from_numpy(init))
    rc = lib.shdr_conv2d_wgrad_x3_f32(ctypes.byref(d), P(xh), P(xl), which, P(zh), P(zl), P(xs), P(zs), P(dw), K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    guards_intact(buf, init.size, what)
    same(dw.cpu().numpy(), want, "%s (source %d, low plane of %s; the other rows untouched)" % (what, which, fine), tile)


def x3_tile(cx, cz):
    return (128 if cx % 128 == 0 or cx % 128 > 64 else 64, 128 if cz % 128 == 0 else 64)


TX_FINE, B_FINE = 7, 8.0                                                  # the fine operand: slot 8.0 -> T = 7
# id, n, h, w, c1, c2, cout, k, stride, x2s, accumulate
X3_CASES = [
    ("x3_128x128_cx128_cz128_pixels_1", 1, 1, 1, 128, 0, 128, 3, 1, 1.0, False),
    ("x3_128x64_cx128_cz64_pixels_33", 1, 3, 11, 128, 0, 64, 3, 1, 1.0, False),
    ("x3_64x128_cx64_cz128_pixels_33", 1, 3, 11, 64, 0, 128, 3, 1, 1.0, False),
    ("x3_64x64_cx64_cz64_pixels_1650", 1, 33, 50, 64, 0, 64, 3, 1, 1.0, False),
    ("x3_128x128_cx96_zero_quarter_cz128", 1, 3, 11, 96, 0, 128, 3, 1, 1.0, False),
    ("x3_128x64_cx96_cz192_k7_s2_stem", 1, 33, 50, 96, 0, 192, 7, 2, 1.0, False),
    ("x3_64x64_cx160_ragged_tile_cz64", 1, 3, 11, 160, 0, 64, 3, 1, 1.0, False),
    ("x3_64x128_cx192_cz128_s2", 2, 9, 13, 192, 0, 128, 3, 2, 1.0, False),
    ("x3_64x64_cx192_cz192_pixels_1", 1, 1, 1, 192, 0, 192, 3, 1, 1.0, False),
    ("x3_128x128_cx128_cz128_pixels_1650_slices", 1, 33, 50, 128, 0, 128, 3, 1, 1.0, False),
    ("x3_128x64_cx128_cz64_k7", 1, 5, 13, 128, 0, 64, 7, 1, 1.0, False),
    ("x3_two_sources_96_64_guard_rows_inside", 1, 3, 11, 96, 64, 64, 3, 1, S8, False),
    ("x3_two_sources_160_64_guard_rows_inside", 1, 5, 13, 160, 64, 128, 3, 1, 0.5, False),
    ("x3_two_sources_64_128_scaled_1650", 1, 33, 50, 64, 128, 64, 3, 1, S8, False),
    ("x3_accumulate_64_64_slices", 1, 33, 50, 64, 0, 64, 3, 1, 1.0, True),
    ("x3_accumulate_two_sources_128_64_s2", 2, 9, 13, 128, 64, 128, 3, 2, 0.5, True),
]


@pytest.mark.parametrize("fine", ["x", "dz"])
@pytest.mark.parametrize("case", X3_CASES, ids=[c[0] for c in X3_CASES])
def test_split_operand_kernel(K, lib, case, fine):
    """`fine` names the operand with the non-empty low plane: "x" tests the cross term Xl Zh alone, "dz" the term Xh Zl alone.  The
    coarse operand is an integer tensor e 2^m under the slot 2^(m + 1): its high plane is 512 e, its low plane empty.  The slots of x
    and dz differ (T = 7 and T = 9 - m)."""
    name, n, h, w, c1, c2, cout, k, stride, x2s, accumulate = case
    rng = np.random.default_rng(len(name) * 7 + h + (fine == "dz"))
    ho, wo = -(-h // stride), -(-w // stride)
    npix = n * ho * wo
    ct = c1 + c2
    d = desc_of(K, (n, h, w, c1), c2, k, cout, stride, x2s)
    if fine == "dz":
        dz, zk, zj = fine_operand(rng, (n, ho, wo, cout), TX_FINE)
        z_bound = B_FINE
    else:
        dz, z_bound = ints(rng, (n, ho, wo, cout), -2, 2), 2.0
    buf, v = guarded(k * k * ct * cout)
    dw = v.view(torch.float32).view(k, k, ct, cout)
    for which, cx, off, s in ((0, c1, 0, 1.0),) + (((1, c2, c1, x2s),) if c2 else ()):
        assert lib.shdr_conv2d_wgrad_x3_ok_f32(ctypes.byref(d), which) == 1
        if fine == "x":
            src, xk, xj = fine_operand(rng, (n, h, w, cx), TX_FINE)
            src, x_bound = src / s, B_FINE / s                          # the scale of the second source is a power of two
        else:
            src, x_bound = ints(rng, (n, h, w, cx), -2, 2) / s, 2.0 / s
        unit = 2.0 ** -(TX_FINE + 11)                                    # of dW = s * sum src dz = 2^-7 sum (k + j 2^-11) e
        # the planes are what the argument says they are
        fh, fl = C.split_planes(src if fine == "x" else dz, x_bound if fine == "x" else z_bound)
        eh, el = C.split_planes(dz if fine == "x" else src, z_bound if fine == "x" else x_bound)
        fk, fj = (xk, xj) if fine == "x" else (zk, zj)
        assert np.array_equal(fh.astype(np.float64), fk) and np.array_equal(fl.astype(np.float64), fj) and fl.any()
        coarse = (dz if fine == "x" else src * s)
        assert np.array_equal(eh.astype(np.float64), 512.0 * coarse) and not el.any()
        ref = C.wgrad_split(src, dz, (k, k), stride, x_bound, z_bound, s)
        assert np.array_equal(ref, C.wgrad(src, None, dz, (k, k, cx, cout), stride, 1.0, None) * s), "the model is exact here"
        # value = unit * (2048 sum k e + sum j e): <= npix terms of magnitude <= 2048 * 4 + 4 units, plus the caller's content
        base = base_of((k, k, cx, cout), accumulate, cx + cout).astype(np.float64) * unit * 2048.0
        assert npix < 2048 and npix * (2048 * 4 + 4) + float(np.abs(base).max(initial=0.0)) / unit < LIMIT
        assert np.array_equal(ref / unit, np.rint(ref / unit))
        init = forbidden((k, k, ct, cout))
        init[:, :, off:off + cx] = base.astype(np.float32)
        want = init.copy()
        want[:, :, off:off + cx] = (base + ref).astype(np.float32)
        assert np.array_equal(want[:, :, off:off + cx].astype(np.float64), base + ref)
        run_x3_source(K, lib, d, which, src, dz, x_bound, z_bound, fine, dw, buf, init, want, name, x3_tile(cx, cout))


def test_split_operand_kernel_refusals(K, lib, monkeypatch):
    n, h, w = 1, 3, 11
    planes = torch.zeros((n * h * w * 192 + 8,), device="cuda", dtype=torch.float16)
    buf, dw = guarded(9 * 192 * 192)
    sl = slot_of(2.0)
    st = K._stream()

    def call(d, which=0, xh=planes, xl=planes, zh=planes, zl=planes, off=0):
        return lib.shdr_conv2d_wgrad_x3_f32(ctypes.byref(d), P(xh, off), P(xl), which, P(zh), P(zl), P(sl), P(sl), P(dw), st)

    good = desc_of(K, (n, h, w, 64), 0, 3, 64, 1)
    assert lib.shdr_conv2d_wgrad_x3_ok_f32(ctypes.byref(good), 0) == 1
    for what, d in (("Cx = 32", desc_of(K, (n, h, w, 32), 0, 3, 64, 1)), ("Cx = 80", desc_of(K, (n, h, w, 80), 0, 3, 64, 1)),
                    ("Cout = 96", desc_of(K, (n, h, w, 64), 0, 3, 96, 1)), ("cout_valid < Cout", desc_of(K, (n, h, w, 64), 0, 3, 64, 1, cout=128)),
                    ("second source of 32", desc_of(K, (n, h, w, 64), 32, 3, 64, 1))):
        which = 1 if what.startswith("second") else 0
        assert lib.shdr_conv2d_wgrad_x3_ok_f32(ctypes.byref(d), which) == 0, what
        assert call(d, which) == E_SHAPE, (what, lib.shdr_last_error())
        untouched(buf, what)
    assert call(good, off=8) == E_ALIGN
    untouched(buf, "xh misaligned")
    for name in ("SHDR_NO_WGRAD_X3", "SHDR_NO_X3"):
        monkeypatch.setenv(name, "1")
        assert lib.shdr_conv2d_wgrad_x3_ok_f32(ctypes.byref(good), 0) == 0 and call(good) == E_SHAPE, name
        untouched(buf, name)
        monkeypatch.delenv(name)
    assert lib.shdr_conv2d_wgrad_x3_ok_f32(ctypes.byref(good), 0) == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_bias_grad_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def bias_lanes(c):
    cl = 1
    while cl < c and cl < 256:
        cl <<= 1
    return 256 // cl                                                     # PL: pixel lanes of a block; one block per PL * 64 pixels


BIAS = []
for _c in (1, 3, 16, 48, 256, 300, 1024):
    _e = bias_lanes(_c) * 64
    for _i, _npix in enumerate((1, _e - 1, _e, _e + 1)):
        BIAS.append((_c, _npix, _i == 3))
BIAS.append((256, 65537, True))                                          # one pixel past the cap of 1024 blocks (PL = 1)
BIAS = sorted(set(BIAS))


@pytest.mark.parametrize("c,npix,accumulate", BIAS, ids=["c%d_npix%d%s" % (c, p, "_acc" if a else "") for c, p, a in BIAS])
def test_bias_gradient(K, lib, c, npix, accumulate):
    g = torch.Generator(device="cuda").manual_seed(c * 31 + npix)
    dzd = torch.randint(-2, 3, (npix, c), device="cuda", generator=g, dtype=torch.int32).float()
    dz = dzd.cpu().numpy().astype(np.float64)
    ref = C.bias_grad(dz)
    base = base_of((c,), accumulate, c + npix)
    small_ints(dz, 1.0, "dz")
    assert 2 * npix + float(np.abs(base).max(initial=0.0)) < LIMIT
    buf, v = guarded(c)
    db = v.view(torch.float32)
    db.copy_(torch.from_numpy(base))
    rc = lib.shdr_bias_grad_f32(P(dzd), P(db), npix, c, K._stream())
    assert rc == 0, (rc, lib.shdr_last_error())
    guards_intact(buf, c, "db")
    same(db.cpu().numpy(), (base.astype(np.float64) + ref).astype(np.float32), "db")


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_filter_transform_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def any_bits(rng, shape):
    """arbitrary fp32 bit patterns, denormals and infinities included; NaN patterns (whose payload a product need not keep) are
    turned into finite numbers"""
    b = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
    b[nan] &= np.uint32(0xBFFFFFFF)
    flat = b.reshape(-1)
    flat[0::53] &= np.uint32(0x807FFFFF)                                 # denormals
    flat[1::211] = 0x7F800000
    flat[2::211] = 0xFF800000
    flat[3::211] = 0x80000000
    return b.view(np.float32)


# kh, kw, cin, cout, c_begin, c_count, scale
FILTER = [(1, 1, 16, 8, 0, 16, 1.0), (3, 3, 16, 32, 0, 16, 1.0), (7, 7, 3, 5, 0, 3, 0.5), (3, 4, 24, 7, 8, 9, S8), (3, 3, 48, 16, 32, 16, S8),
          (1, 1, 5, 3, 4, 1, -2.0), (7, 7, 96, 64, 32, 33, 0.5), (4, 3, 6, 300, 1, 4, 1.0)]


@pytest.mark.parametrize("case", FILTER, ids=["%dx%d_%d_%d_rows_%d+%d_scale_%g" % c for c in FILTER])
def test_filter_transform(K, lib, case):
    kh, kw, cin, cout, c_begin, c_count, scale = case
    w = any_bits(np.random.default_rng(kh * 100 + cin), (kh, kw, cin, cout))
    with np.errstate(over="ignore", invalid="ignore"):
        want = C.filter_transform(w, c_begin, c_count, scale).astype(np.float32)     # a power-of-two scale: ONE rounding, in denormals only
    assert not np.isnan(want).any()
    numel = kh * kw * cout * c_count
    buf, v = guarded(numel)
    wd = torch.from_numpy(w).cuda()
    rc = lib.shdr_filter_transform_f32(P(wd), P(v), kh, kw, cin, cout, c_begin, c_count, scale, K._stream())
    assert rc == 0, (rc, lib.shdr_last_error())
    guards_intact(buf, numel, "wt")
    same(v.view(torch.float32).view(kh, kw, cout, c_count).cpu().numpy(), want, "wt")
    got = K.filter_transform(wd, c_begin, c_count, scale)                # the wrapper is the same call
    assert torch.equal(got.view(torch.int32).view(-1), v)


# ---------------------------------------------------------------------------------------------------------------------------------
# argument refusals of the five entry points: the documented code, and nothing written
# ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_leave_the_outputs_untouched(K, lib):
    n, h, w, c, cout = 1, 3, 11, 64, 64
    x = torch.zeros((n * h * w * c + 4,), device="cuda")
    dz = torch.zeros((n * h * w * cout + 4,), device="cuda")
    planes = torch.zeros((n * h * w * c + 8,), device="cuda", dtype=torch.float16)
    sl = slot_of(2.0)
    buf, dw = guarded(9 * 2 * c * cout)
    dubuf, du = guarded(16 * c * cout)
    st = K._stream()

    def desc(**kw):
        d = desc_of(K, (n, h, w, kw.pop("c1", c)), kw.pop("c2", 0), 3, cout, 1)
        for k_, v_ in kw.items():
            setattr(d, k_, v_)
        return d

    def refused(rc, code, what):
        assert rc == code, (what, rc, code, lib.shdr_last_error())
        untouched(buf, what)
        untouched(dubuf, what)

    dims = ("N", "H", "W", "KH", "KW", "stride", "Ho", "Wo")
    # shdr_conv2d_wgrad_f32
    wg = lib.shdr_conv2d_wgrad_f32
    refused(wg(None, P(x), 0, P(dz), P(dw), st), E_NULL, "wgrad: null descriptor")
    refused(wg(ctypes.byref(desc()), None, 0, P(dz), P(dw), st), E_NULL, "wgrad: null x")
    refused(wg(ctypes.byref(desc()), P(x), 0, None, P(dw), st), E_NULL, "wgrad: null dz")
    refused(wg(ctypes.byref(desc()), P(x), 0, P(dz), None, st), E_NULL, "wgrad: null dw")
    refused(wg(ctypes.byref(desc()), P(x), 2, P(dz), P(dw), st), E_SHAPE, "wgrad: which = 2")
    refused(wg(ctypes.byref(desc()), P(x), -1, P(dz), P(dw), st), E_SHAPE, "wgrad: which = -1")
    refused(wg(ctypes.byref(desc()), P(x), 1, P(dz), P(dw), st), E_SHAPE, "wgrad: second source without C2")
    for f in dims + ("C1", "Cout"):
        for bad in (0, -1):
            refused(wg(ctypes.byref(desc(**{f: bad, "cout_valid": 0})), P(x), 0, P(dz), P(dw), st), E_SHAPE, "wgrad: %s = %d" % (f, bad))
    # shdr_conv2d_wgrad_winograd_f32
    wino = lib.shdr_conv2d_wgrad_winograd_f32
    ok = [P(x), P(dz), P(du), P(dw), n, h, w, c, cout, c, 0, 1.0]
    for i, what in enumerate(("x", "dz", "du", "dw")):
        args = list(ok)
        args[i] = None
        refused(wino(*args, st), E_NULL, "winograd: null " + what)
    for i, what in ((4, "N"), (5, "H"), (6, "W"), (7, "Cx"), (8, "Cout")):
        for bad in (0, -1):
            args = list(ok)
            args[i] = bad
            refused(wino(*args, st), E_SHAPE, "winograd: %s = %d" % (what, bad))
    # shdr_conv2d_wgrad_x3_f32
    x3 = lib.shdr_conv2d_wgrad_x3_f32
    okx = [ctypes.byref(desc()), P(planes), P(planes), 0, P(planes), P(planes), P(sl), P(sl), P(dw)]
    for i, what in ((0, "descriptor"), (1, "xh"), (2, "xl"), (4, "zh"), (5, "zl"), (6, "x range"), (7, "dz range"), (8, "dw")):
        args = list(okx)
        args[i] = None
        refused(x3(*args, st), E_NULL, "x3: null " + what)
    for which, what in ((2, "which = 2"), (-1, "which = -1"), (1, "second source without C2")):
        args = list(okx)
        args[3] = which
        refused(x3(*args, st), E_SHAPE, "x3: " + what)
    for f in dims + ("C1", "Cout"):
        for bad in (0, -1):
            args = list(okx)
            args[0] = ctypes.byref(desc(**{f: bad, "cout_valid": 0 if f == "Cout" else cout}))
            refused(x3(*args, st), E_SHAPE, "x3: %s = %d" % (f, bad))
    for which, other in ((0, {"C2": -64}), (1, {"C2": 64, "C1": 0}), (1, {"C2": 64, "C1": -64})):     # a bad count in the OTHER source
        args = list(okx)
        args[0], args[3] = ctypes.byref(desc(**other)), which
        refused(x3(*args, st), E_SHAPE, "x3: source %d with %r" % (which, other))
    # shdr_bias_grad_f32 (db = the guarded dw buffer)
    bg = lib.shdr_bias_grad_f32
    refused(bg(None, P(dw), 8, 16, st), E_NULL, "bias_grad: null dz")
    refused(bg(P(dz), None, 8, 16, st), E_NULL, "bias_grad: null db")
    for npix, ch in ((0, 16), (-1, 16), (8, 0), (8, -3)):
        refused(bg(P(dz), P(dw), npix, ch, st), E_SHAPE, "bias_grad: npix = %d, C = %d" % (npix, ch))
    # shdr_filter_transform_f32 (wt = the guarded dw buffer)
    ft = lib.shdr_filter_transform_f32
    refused(ft(None, P(dw), 3, 3, 16, 16, 0, 16, 1.0, st), E_NULL, "filter_transform: null w")
    refused(ft(P(x), None, 3, 3, 16, 16, 0, 16, 1.0, st), E_NULL, "filter_transform: null wt")
    for what, a in (("KH = 0", (0, 3, 16, 16, 0, 16)), ("KW = -1", (3, -1, 16, 16, 0, 16)), ("Cin = 0", (3, 3, 0, 16, 0, 16)),
                    ("Cout = 0", (3, 3, 16, 0, 0, 16)), ("c_begin < 0", (3, 3, 16, 16, -1, 16)), ("c_count = 0", (3, 3, 16, 16, 0, 0)),
                    ("rows past Cin", (3, 3, 16, 16, 8, 9))):
        refused(ft(P(x), P(dw), *a, 1.0, st), E_SHAPE, "filter_transform: " + what)
