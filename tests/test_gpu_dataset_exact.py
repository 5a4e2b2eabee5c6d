"""The training-set reader kernels (csrc/dataset.hip: hdr_load_resize, hdr_window_partials, hdr_window_fold, hdr_patch_sample;
csrc/exr.hip: exr_load_resize) through the C ABI against the float32 restatement tests/dataset_ref.py, BIT FOR BIT.

Both files are compiled with -ffp-contract=off and state cv2's bilinear map operation for operation as dataset_ref._axis /
resize_linear do: the tap positions come from the same float64 expression rounded once to float32, the weights from one float32
subtraction, each blend is two products and a sum, the patch normalisation is one product and one correctly rounded division.
Nothing is left to excuse a difference, so the bar is equality of bit patterns (NaN compared as NaN where a source holds inf or NaN:
an inf tap under a zero weight is NaN on both sides).  Sources are a few pixels large; one case per entry point lies past the
2048-block cap of shdr::stream_grid.  Outputs sit between guard words; after each ABI case the _ops wrapper returns the same bits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dataset_ref as R
import tape_ref as T
from test_gpu_conv_x3_exact import E_ALIGN, E_NULL, E_SHAPE
from test_gpu_wgrad_f32_exact import P, guarded, guards_intact, same, untouched

pytestmark = pytest.mark.gpu

HALF, FLOAT = 1, 2                          # SHDR_EXR_HALF, SHDR_EXR_FLOAT (OpenEXR's pixel types)
WIN = 512
CNT = WIN * WIN * 3

# (H0, W0) -> (H, W)
RESIZE = [((7, 9), (7, 9), "identity"), ((16, 24), (8, 12), "2x down"), ((5, 7), (10, 14), "2x up"),
          ((13, 17), (9, 31), "non-integer"), ((9, 31), (13, 17), "non-integer"),
          ((1, 1), (4, 5), "gap 9: one-pixel axes"), ((1, 9), (3, 3), "gap 9: one-pixel axis"), ((9, 1), (3, 3), "gap 9: one-pixel axis"),
          ((2, 2), (7, 7), "gap 9: two-pixel axes"), ((64, 96), (3, 5), "large downscale"),
          ((37, 53), (600, 900), "gap 7: 540 000 pixels, past the 2048 x 256 grid cap")]
RESIZE_IDS = ["%dx%d-%dx%d" % (a + b) for a, b, _ in RESIZE]


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def f32_out(numel):
    buf, view = guarded(numel)
    return buf, view.view(torch.float32)


def same_or_nan(got, want, what):
    """bit patterns equal, except that a NaN answers a NaN whatever its payload"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN in different places"
    same(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), what)


# ---------------------------------------------------------------------------------------------------------------------------------
# B1  shdr_hdr_load_resize_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def rgbe_source(h, w):
    """RGBE bytes whose exponents include 0 (black), 1 and 9 (subnormal and smallest normal floats), 128 and 255, and whose
    mantissas include 0 and 255"""
    rng = np.random.default_rng(1000 * h + w)
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    e = rng.integers(110, 150, size=(h, w))
    pick = rng.random((h, w))
    for i, v in enumerate((0, 1, 9, 128, 255)):
        e[(pick >= 0.08 * i) & (pick < 0.08 * (i + 1))] = v
    img[..., 3] = e
    ext = rng.random((h, w, 3))
    img[..., :3][ext < 0.05] = 0
    img[..., :3][ext > 0.95] = 255
    if h * w >= 7:
        flat = img.reshape(-1, 4)
        flat[:5, 3] = (0, 1, 9, 128, 255)
        flat[1, :3] = (255, 0, 1)
        flat[5] = (255, 255, 255, 1)
        flat[6] = (0, 0, 0, 255)
    return img


@pytest.mark.parametrize("case", RESIZE, ids=RESIZE_IDS)
def test_hdr_load_resize(K, lib, case):
    """gaps 7 and 9: the Radiance loader through the ABI at every clamp rule of linear_taps, subnormal decoded values included"""
    (h0, w0), (h, w), _ = case
    img = rgbe_source(h0, w0)
    bgr = R.rgbe_bgr(img)
    if h0 * w0 >= 7:
        assert (0 < bgr).any() and (bgr[bgr > 0] < np.finfo(np.float32).tiny).any(), "no subnormal source value"
    want, _ = R.resize_linear(bgr, (h, w))
    src = dev(img)
    buf, y = f32_out(h * w * 3)
    rc = lib.shdr_hdr_load_resize_f32(P(src), P(y), h0, w0, h, w, stream())
    assert rc == 0, lib.shdr_last_error()
    guards_intact(buf, h * w * 3, "hdr_load_resize")
    got = y.view(h, w, 3).cpu().numpy()
    same(got, want, "hdr_load_resize %s" % (case,))
    if (h0, w0) == (h, w):
        same(got, bgr, "identity is a copy")
    again = K.hdr_load_resize(src, torch.empty((h, w, 3), device="cuda"))
    same(again.cpu().numpy(), want, "wrapper")


def test_hdr_load_resize_refusals(lib):
    src = dev(rgbe_source(8, 8))
    pad = torch.zeros(8 * 8 * 4 + 4, dtype=torch.uint8, device="cuda")
    buf, y = f32_out(4 * 4 * 3)
    st = stream()
    assert pad.data_ptr() % 4 == 0
    assert lib.shdr_hdr_load_resize_f32(P(pad, 1), P(y), 8, 8, 4, 4, st) == E_ALIGN
    for dims in ((0, 8, 4, 4), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 4, 0), (-1, 8, 4, 4)):
        assert lib.shdr_hdr_load_resize_f32(P(src), P(y), *dims, st) == E_SHAPE
    assert lib.shdr_hdr_load_resize_f32(None, P(y), 8, 8, 4, 4, st) == E_NULL
    assert lib.shdr_hdr_load_resize_f32(P(src), None, 8, 8, 4, 4, st) == E_NULL
    untouched(buf, "hdr_load_resize")


# ---------------------------------------------------------------------------------------------------------------------------------
# B2  shdr_exr_load_resize_f32
# ---------------------------------------------------------------------------------------------------------------------------------
HALF_SPECIALS = [0x8000, 0xBC00, 0xC500, 0x0001, 0x03FF, 0x8200, 0x7C00, 0xFC00, 0x7C01, 0x7E00, 0xFE55]
FLOAT_SPECIALS = [0x80000000, 0xBF800000, 0xC0A00000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7F802000, 0x7FC00000, 0xFFC12345]


def exr_source(h0, w0, types, lines, seed):
    """(bytes, chunk offsets [n_chunks + 1], row_bytes, chan_off, converted float32 [h0, w0, 3]).

    A scanline is four planar runs: an extra HALF channel first (inside row_bytes, never addressed), then the three colour runs in
    the order 2, 1, 0 (a B, G, R table: output channel 0 is the LAST run).  Chunks of `lines` scanlines (the last one partial) are
    stored in DECREASING y order with gaps of junk bytes between them.  Samples: random values, and where the source has room -0,
    negatives, subnormals, +-inf and NaN payloads (quiet and signalling)."""
    rng = np.random.default_rng(seed)
    planes, conv = [], []
    for t in types:
        if t == HALF:
            b = rng.normal(0.0, 3.0, (h0, w0)).astype(np.float16).view(np.uint16).copy()
            sp = np.array(HALF_SPECIALS, dtype=np.uint16)
        else:
            b = rng.normal(0.0, 3.0, (h0, w0)).astype(np.float32).view(np.uint32).copy()
            sp = np.array(FLOAT_SPECIALS, dtype=np.uint32)
        k = min(len(sp), h0 * w0 // 6)
        b.reshape(-1)[rng.choice(h0 * w0, size=k, replace=False)] = sp[rng.permutation(len(sp))[:k]]
        planes.append(b)
        conv.append(R.half_bits_to_float(b) if t == HALF else b.view(np.float32))
    extra = np.full((h0, w0), 0x3C00, dtype=np.uint16)
    runs = [extra, planes[2], planes[1], planes[0]]
    sizes = [r.dtype.itemsize * w0 for r in runs]
    row_bytes = sum(sizes)
    chan_off = [sum(sizes[:3]), sum(sizes[:2]), sizes[0]]
    rows = [b"".join(r[y].tobytes() for r in runs) for y in range(h0)]
    n_chunks = -(-h0 // lines)
    offsets = np.zeros(n_chunks + 1, dtype=np.int64)
    data = b""
    for ck in range(n_chunks - 1, -1, -1):
        data += b"\xee" * (5 + ck % 3)
        offsets[ck] = len(data)
        data += b"".join(rows[ck * lines:(ck + 1) * lines])
    data += b"\xee" * 3
    offsets[n_chunks] = len(data)
    return np.frombuffer(data, dtype=np.uint8).copy(), offsets, row_bytes, chan_off, np.stack(conv, -1)


def call_exr(lib, planes, offsets, n_chunks, lines, row_bytes, chan_off, types, h0, w0, y, h, w, clip):
    off = (ctypes.c_int64 * 3)(*chan_off)
    typ = (ctypes.c_int32 * 3)(*types)
    return lib.shdr_exr_load_resize_f32(P(planes), planes.numel(), P(offsets), n_chunks, lines, row_bytes, off, typ, h0, w0, P(y), h, w,
                                        clip, stream())


TYPES = [(HALF, HALF, HALF), (FLOAT, FLOAT, FLOAT), (HALF, FLOAT, HALF)]


@pytest.mark.parametrize("case", RESIZE, ids=RESIZE_IDS)
def test_exr_load_resize(K, lib, case):
    """gaps 7 and 9 for the OpenEXR loader: every channel-type table, 1, 3 and 16 lines per chunk (a partial last chunk, gaps, chunks
    stored in decreasing y), clip 0 and 1.  Same-size loads return the stored samples bit for bit (-0 and NaN payloads kept, an inf
    neighbour contaminates nothing); resizes equal resize_linear of the converted planes"""
    (h0, w0), (h, w), _ = case
    saw_special = False
    for ti, types in enumerate(TYPES):
        for lines in (1, 3, 16):
            planes, offsets, row_bytes, chan_off, conv = exr_source(h0, w0, types, lines, seed=97 * h0 + w0 + ti)
            n_chunks = offsets.size - 1
            assert n_chunks == -(-h0 // lines) and (n_chunks < 2 or offsets[0] > offsets[1])
            pd, od = dev(planes), dev(offsets)
            for clip in (0, 1):
                what = "exr_load_resize %s types %s lines %d clip %d" % (case[:2], types, lines, clip)
                src = R.clip0(conv) if clip else conv
                if clip:
                    assert not (src < 0).any()
                with np.errstate(all="ignore"):
                    want = src if (h0, w0) == (h, w) else R.resize_linear(src, (h, w))[0]
                buf, y = f32_out(h * w * 3)
                rc = call_exr(lib, pd, od, n_chunks, lines, row_bytes, chan_off, types, h0, w0, y, h, w, clip)
                assert rc == 0, (what, lib.shdr_last_error())
                guards_intact(buf, h * w * 3, what)
                got = y.view(h, w, 3).cpu().numpy()
                if (h0, w0) == (h, w):
                    same(got, want, what)                              # payloads and signs of zero included
                    u = got.view(np.uint32)
                    saw_special |= bool((u == 0x80000000).any() and np.isinf(got).any() and np.isnan(got).any())
                else:
                    same_or_nan(got, want, what)
                again = K.exr_load_resize(pd, od, lines, row_bytes, chan_off, types, h0, w0, torch.empty((h, w, 3), device="cuda"),
                                          clip=bool(clip))
                same_or_nan(again.cpu().numpy(), got, what + " wrapper")
    assert saw_special == ((h0, w0) == (h, w))


def test_exr_load_resize_refusals(lib):
    types = (HALF, FLOAT, HALF)
    planes, offsets, row_bytes, chan_off, _ = exr_source(7, 9, types, 3, seed=1)
    pd, od = dev(planes), dev(offsets)
    buf, y = f32_out(7 * 9 * 3)
    ok = dict(n_chunks=3, lines=3, row_bytes=row_bytes, chan_off=chan_off, types=types, h0=7, w0=9, h=7, w=9)

    def call(**kw):
        a = dict(ok, **kw)
        return call_exr(lib, pd, od, a["n_chunks"], a["lines"], a["row_bytes"], a["chan_off"], a["types"], a["h0"], a["w0"], y, a["h"],
                        a["w"], 0)
    assert call(n_chunks=2) == E_SHAPE and call(n_chunks=4) == E_SHAPE                   # ceil(7 / 3) = 3
    assert b"chunks" in lib.shdr_last_error()
    assert call(chan_off=[chan_off[0] + 1, chan_off[1], chan_off[2]]) == E_SHAPE          # the last run would end past the scanline
    assert b"does not fit" in lib.shdr_last_error()
    assert call(chan_off=[-1, chan_off[1], chan_off[2]]) == E_SHAPE
    assert call(row_bytes=row_bytes - 1) == E_SHAPE
    assert call(types=(HALF, 0, HALF)) == E_SHAPE and call(types=(3, FLOAT, HALF)) == E_SHAPE   # UINT and an unknown type
    assert b"HALF or FLOAT" in lib.shdr_last_error()
    assert call(lines=0) == E_SHAPE and call(h=0) == E_SHAPE and call(w0=0) == E_SHAPE
    off = (ctypes.c_int64 * 3)(*chan_off)
    typ = (ctypes.c_int32 * 3)(*types)
    st = stream()
    assert lib.shdr_exr_load_resize_f32(None, planes.size, P(od), 3, 3, row_bytes, off, typ, 7, 9, P(y), 7, 9, 0, st) == E_NULL
    assert lib.shdr_exr_load_resize_f32(P(pd), planes.size, None, 3, 3, row_bytes, off, typ, 7, 9, P(y), 7, 9, 0, st) == E_NULL
    assert lib.shdr_exr_load_resize_f32(P(pd), planes.size, P(od), 3, 3, row_bytes, None, typ, 7, 9, P(y), 7, 9, 0, st) == E_NULL
    assert lib.shdr_exr_load_resize_f32(P(pd), planes.size, P(od), 3, 3, row_bytes, off, typ, 7, 9, None, 7, 9, 0, st) == E_NULL
    untouched(buf, "exr_load_resize")
    assert call() == 0
    guards_intact(buf, 7 * 9 * 3, "exr_load_resize")


# ---------------------------------------------------------------------------------------------------------------------------------
# the arena: 512 x 512, 512 x 530 (landscape: windows at columns 0 and 18), 540 x 512 (portrait: windows at rows 0 and 28)
# ---------------------------------------------------------------------------------------------------------------------------------
DIMS = [(512, 512), (512, 530), (540, 512)]


def origin(f, parity):
    h, w = DIMS[f]
    return ((h - WIN if h > w and parity else 0), (w - WIN if h <= w and parity else 0))


def arena_tables():
    sizes = [h * w * 3 for h, w in DIMS]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return offsets, np.array(DIMS, dtype=np.int32), int(sum(sizes))


def split(arena):
    offsets, _, _ = arena_tables()
    return [arena[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offsets, DIMS)]


@functools.lru_cache(maxsize=None)
def hdr_arena():
    """random HDR-like values (log-normal over five decades, a black block, a bright corner), built once and left unchanged"""
    _, _, total = arena_tables()
    rng = np.random.default_rng(77)
    arena = np.exp(rng.normal(0.0, 2.5, total)).astype(np.float32)
    for img in split(arena):
        img[100:140, 200:260] = 0.0
        img[:7, :5] *= 1e4
    arena.setflags(write=False)
    return arena


@functools.lru_cache(maxsize=None)
def integer_arena(parity):
    """integers 0..15 inside the windows of `parity`; every line outside them holds 1e6, so a wrong window origin shows"""
    _, _, total = arena_tables()
    rng = np.random.default_rng(78 + parity)
    arena = rng.integers(0, 16, size=total).astype(np.float32)
    for f, img in enumerate(split(arena)):
        r0, c0 = origin(f, parity)
        mask = np.ones(img.shape[:2], dtype=bool)
        mask[r0:r0 + WIN, c0:c0 + WIN] = False
        img[mask] = 1e6
    arena.setflags(write=False)
    return arena


@pytest.fixture(scope="module")
def tables():
    offsets, dims, _ = arena_tables()
    return dev(offsets), dev(dims)


def run_means(lib, arena_d, tables, what):
    n = len(DIMS)
    pb, part = f32_out(2 * n * 64)
    mb, means = f32_out(2 * n)
    rc = lib.shdr_hdr_window_means_f32(P(arena_d), P(tables[0]), P(tables[1]), n, P(part), P(means), stream())
    assert rc == 0, (what, lib.shdr_last_error())
    guards_intact(pb, 2 * n * 64, what + " partials")
    guards_intact(mb, 2 * n, what + " means")
    return means.clone(), part.clone()


# ---------------------------------------------------------------------------------------------------------------------------------
# B3  shdr_hdr_window_means_f32
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1])
def test_window_means_of_integers_are_exact(K, lib, tables, parity):
    """gap 7: integers 0..15 sum to at most 15 * 786 432 < 2^24, so every float32 partial sum is exact in any order and the mean is
    float32(sum) / float32(786432), one correctly rounded division; lines outside the window hold 1e6"""
    arena = integer_arena(parity)
    ad = dev(arena)
    means, part = run_means(lib, ad, tables, "integer arena")
    means, part = means.cpu().numpy(), part.cpu().numpy().reshape(6, 64)
    for f, img in enumerate(split(arena)):
        r0, c0 = origin(f, parity)
        win = img[r0:r0 + WIN, c0:c0 + WIN].astype(np.int64)
        assert win.max() <= 15 and (f == 0 or (img == 1e6).any())
        want = np.float32(win.sum()) / np.float32(CNT)
        assert means[2 * f + parity] == want, (f, parity, means[2 * f + parity], want)
        assert np.array_equal(part[2 * f + parity], win.reshape(64, -1).sum(axis=1).astype(np.float32)), (f, parity)
    again = K.hdr_window_means(ad, *tables).cpu().numpy()
    assert np.array_equal(again[parity::2].view(np.uint32), means[parity::2].view(np.uint32))


# depth of the two-stage tree above one value: (a + b) + c of its pixel (2), the thread's chain over its 16 pixels (16), the 256-thread
# LDS tree (8), the fold of the 64 partials (6): every value passes at most 32 float32 additions, then one division
TREE_DEPTH = 2 + 16 + 8 + 6


def test_window_means_of_hdr_values(K, lib, tables):
    """against float64 at the count of the tree: |mean - ref| <= (32 + 1) 2^-24 mean|x| (tape_ref.bar32, the per-path form of
    tape_ref.sum_bar: no value passes more than 32 additions); two launches give the same bits"""
    arena = hdr_arena()
    ad = dev(arena)
    means, part = run_means(lib, ad, tables, "hdr arena")
    again, part2 = run_means(lib, ad, tables, "hdr arena again")
    assert torch.equal(means.view(torch.int32), again.view(torch.int32)) and torch.equal(part.view(torch.int32), part2.view(torch.int32))
    m = means.cpu().numpy()
    worst = 0.0
    for f, img in enumerate(split(arena)):
        for parity in (0, 1):
            r0, c0 = origin(f, parity)
            win = img[r0:r0 + WIN, c0:c0 + WIN].astype(np.float64)
            ref, bar = win.sum() / CNT, float(T.bar32(TREE_DEPTH + 1, np.abs(win).sum() / CNT))
            err = abs(float(m[2 * f + parity]) - ref)
            worst = max(worst, err / bar)
            assert err <= bar, (f, parity, err, bar)
    print("window means: worst error %.3f of the bar" % worst)
    assert np.array_equal(K.hdr_window_means(ad, *tables).cpu().numpy().view(np.uint32), m.view(np.uint32))


def test_window_means_refusals(lib, tables):
    ad = dev(hdr_arena()[:16])
    pb, part = f32_out(6 * 64)
    mb, means = f32_out(6)
    st = stream()
    assert lib.shdr_hdr_window_means_f32(P(ad), P(tables[0]), P(tables[1]), 0, P(part), P(means), st) == E_SHAPE
    assert lib.shdr_hdr_window_means_f32(P(ad), P(tables[0]), P(tables[1]), -3, P(part), P(means), st) == E_SHAPE
    assert lib.shdr_hdr_window_means_f32(P(ad), P(tables[0]), P(tables[1]), 1 << 30, P(part), P(means), st) == E_SHAPE
    for i in range(5):
        a = [P(ad), P(tables[0]), P(tables[1]), P(part), P(means)]
        a[i] = None
        assert lib.shdr_hdr_window_means_f32(a[0], a[1], a[2], 3, a[3], a[4], st) == E_NULL
    untouched(pb, "partials")
    untouched(mb, "means")


# ---------------------------------------------------------------------------------------------------------------------------------
# B4  shdr_hdr_patch_sample_f32
# ---------------------------------------------------------------------------------------------------------------------------------
MEANS = np.array([0.0, 0.37, 1.5, 1e-3, 7.25, 0.011], dtype=np.float32)         # GIVEN, not computed; 0.0 -> a denominator of 1e-6


def sizes_of(p):
    return [p, p + 1, 256, 257, 511, 512, 513, 700, 1024, 2047, 2048]


def patch_params(p, stride):
    """36 rows per S: every (y0, x0) of {0, (S - P) // 2, S - P}^2 four times and every (k, flip0, flip1) at least twice, in pairs
    that differ from row to row; idx scrambled over the six windows; columns past 7 hold junk"""
    rng = np.random.default_rng(p)
    rows = []
    for S in sizes_of(p):
        pos = [0, (S - p) // 2, S - p]
        idx = rng.permutation(36) % 6
        for r in range(36):
            c = r % 16
            rows.append([int(idx[r]), S, pos[(r % 9) // 3], pos[r % 3], c & 3, (c >> 2) & 1, (c >> 3) & 1] + [7777 + r] * (stride - 7))
        assert {tuple(q[4:7]) for q in rows[-36:]} == {(k, a, b) for k in range(4) for a in (0, 1) for b in (0, 1)}
        assert {tuple(q[2:4]) for q in rows[-36:]} == {(a, b) for a in pos for b in pos} and {q[0] for q in rows[-36:]} == set(range(6))
    return np.array(rows, dtype=np.int32)


@pytest.mark.parametrize("stride", [7, 9])
@pytest.mark.parametrize("p", [16, 48])
def test_patch_sample(K, lib, tables, p, stride):
    """gap 8: patch sides 16 and 48 (one and nine 16 x 16 blocks per sample), `params` of stride 7 and 9, S from P (a 32x downscale)
    to 2048 (a 4x upscale), crops at both ends of both axes, all 16 rotations and flips at every S: every element equals
    dataset_ref.patch_crop bit for bit"""
    arena = hdr_arena()
    imgs = split(arena)
    params = patch_params(p, stride)
    n = len(params)
    ad, pd, md = dev(arena), dev(params), dev(MEANS)
    buf, y = f32_out(n * p * p * 3)
    rc = lib.shdr_hdr_patch_sample_f32(P(ad), P(tables[0]), P(tables[1]), P(md), P(pd), stride, n, len(DIMS), p, P(y), stream())
    assert rc == 0, lib.shdr_last_error()
    guards_intact(buf, n * p * p * 3, "patch_sample")
    got = y.view(n, p, p, 3).cpu().numpy()
    for i, row in enumerate(params.tolist()):
        idx, S, y0, x0, k, f0, f1 = row[:7]
        want, _ = R.patch_crop(imgs[idx // 2], idx, S, y0, x0, k, f0, f1, MEANS[idx], p)
        same(got[i], want, "patch_sample P %d row %d %s" % (p, i, row[:7]))
    again = K.hdr_patch_sample(ad, tables[0], tables[1], md, pd, p)
    same(again.cpu().numpy(), got, "wrapper")


def test_patch_sample_refusals(lib, tables):
    ad, md = dev(hdr_arena()[:16]), dev(MEANS)
    pd = dev(patch_params(16, 7)[:4])
    buf, y = f32_out(4 * 16 * 16 * 3)
    st = stream()

    def call(n=4, stride=7, p=16, files=3, ptrs=None):
        a = ptrs or [P(ad), P(tables[0]), P(tables[1]), P(md), P(pd), P(y)]
        return lib.shdr_hdr_patch_sample_f32(a[0], a[1], a[2], a[3], a[4], stride, n, files, p, a[5], st)
    assert call(p=24) == E_SHAPE and call(p=8) == E_SHAPE and call(p=0) == E_SHAPE        # P % 16
    assert call(p=2064) == E_SHAPE                                                        # P > 2048
    assert call(n=0) == E_SHAPE and call(n=65536) == E_SHAPE and call(files=0) == E_SHAPE
    assert call(stride=6) == E_SHAPE
    for i in range(6):
        a = [P(ad), P(tables[0]), P(tables[1]), P(md), P(pd), P(y)]
        a[i] = None
        assert call(ptrs=a) == E_NULL
    untouched(buf, "patch_sample")
