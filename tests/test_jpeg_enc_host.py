"""CPU tests of the baseline-JPEG writer: the NumPy reference (jpeg_enc_ref.py) and libshdr's host twin (K.jpeg_encode_host and its two
stages, csrc/jpeg_enc.h) each write PIL's file, byte for byte; the entropy stage writes jpeg_synth's scan for coefficients no image
produces; what is out of scope is refused.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

import jpeg_enc_ref as R


def _desc(K, h, w, layout, quality=75, restart=0):
    return K.jpeg_enc_images([(h, w)], quality, layout, restart)


@pytest.fixture(scope="module")
def pil_files():
    """PIL's file for every case of the grid, made once: {(layout, (H, W), quality, content, restart): bytes}"""
    files = {}
    for layout in R.LAYOUTS:
        for size in R.SIZES:
            for q in R.QUALITIES:
                for kind in R.CONTENTS:
                    for rst in R.restart_intervals(size[0], size[1], layout):
                        files[(layout, size, q, kind, rst)] = R.pil_encode(R.content(kind, size[0], size[1], seed=q), layout, q, rst)
    return files


def test_grid_reaches_rstn_wraparound():
    """at least one case of the grid has >= 10 restart segments, so that RSTn wraps from D7 to D0"""
    most = max(-(-mx * my // rst) for layout in R.LAYOUTS for (h, w) in R.SIZES for (mx, my) in [R.mcu_grid(h, w, layout)]
               for rst in R.restart_intervals(h, w, layout) if rst)
    assert most >= 10
    data = R.pil_encode(R.content("noise", 48, 64), "444", 50, 1)
    assert b"\xff\xd7" in data and data.count(b"\xff\xd0") >= 2


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_host_twin_writes_pils_file(shdr, pil_files, layout):
    K = shdr._ops
    for (lay, (h, w), q, kind, rst), want in pil_files.items():
        if lay != layout:
            continue
        got = K.jpeg_encode_host(R.content(kind, h, w, seed=q), _desc(K, h, w, layout, q, rst))
        assert got == want, (layout, h, w, q, kind, rst)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_reference_writes_pils_file(pil_files, layout):
    for (lay, (h, w), q, kind, rst), want in pil_files.items():
        if lay != layout:
            continue
        assert R.encode(R.content(kind, h, w, seed=q), layout, q, rst) == want, (layout, h, w, q, kind, rst)


def test_stages_compose_to_the_file(shdr):
    """header + entropy(transform(pixels)) + EOI is the file, and the transform stage gives the reference's coefficients"""
    K = shdr._ops
    for layout in R.LAYOUTS:
        for (h, w) in ((7, 9), (17, 33), (8, 8), (48, 64)):
            img = R.content("noise", h, w, seed=h)
            d = _desc(K, h, w, layout, 90, 2)
            coef = K.jpeg_encode_transform_host(img, d)
            comps, want = R.coefficients(img, layout, 90)
            assert np.array_equal(coef, R.arena(w, h, layout, want)), (layout, h, w)
            assert coef.shape[0] == K.jpeg_encode_blocks(d)[0]
            assert K.jpeg_encode_header_host(d) == R.header(w, h, layout, 90, 2)
            assert K.jpeg_encode_header_host(d) + K.jpeg_encode_entropy_host(coef, d) + b"\xff\xd9" == K.jpeg_encode_host(img, d)


COEF_CASES = R.coefficient_cases()


@pytest.fixture(scope="module")
def coef_scans():
    return {name: R.scan(w, h, layout, coef, rst) for name, w, h, layout, rst, coef in COEF_CASES}


@pytest.mark.parametrize("case", COEF_CASES, ids=[c[0] for c in COEF_CASES])
def test_entropy_stage_on_coefficients(shdr, coef_scans, case):
    K = shdr._ops
    name, w, h, layout, rst, coef = case
    got = K.jpeg_encode_entropy_host(R.arena(w, h, layout, coef), _desc(K, h, w, layout, 75, rst))
    assert got == coef_scans[name]


def test_stuffing_is_exercised(coef_scans):
    """one reference stream holds at least 10 % FF bytes and two adjacent ones (FF 00 FF 00 once stuffed)"""
    s = coef_scans["constant-1023-444"]
    assert s.count(b"\xff") >= 0.10 * len(s)
    assert b"\xff\x00\xff\x00" in s


def test_out_of_range_coefficients_are_refused(shdr):
    K = shdr._ops
    d = _desc(K, 16, 16, "444")
    coef = np.zeros((12, 64), dtype=np.int16)
    assert len(K.jpeg_encode_entropy_host(coef, d)) > 0
    for block, k, value in ((5, 7, 1024), (4, 63, -1024), (9, 0, 2048), (3, 0, -2048)):
        bad = coef.copy()
        bad[block, k] = value
        with pytest.raises(ValueError, match=r"block %d\b" % block):
            K.jpeg_encode_entropy_host(bad, d)
    ok = coef.copy()
    ok[5, 7], ok[4, 63], ok[9, 0] = 1023, -1023, 2047
    ok[6, 0] = 1023                     # the next block of component 0 (4:4:4: blocks 0, 3, 6, 9): differences 1023 and 1024
    assert len(K.jpeg_encode_entropy_host(ok, d)) > 0
    with pytest.raises(ValueError, match="blocks"):
        K.jpeg_encode_entropy_host(coef[:11], d)


def test_bad_arguments_are_refused(shdr):
    K, jpeg = shdr._ops, shdr.jpeg
    img = np.zeros((8, 8, 3), dtype=np.uint8)
    for kw in (dict(subsampling="440"), dict(subsampling="411"), dict(subsampling=2), dict(quality=0), dict(quality=101), dict(quality=7.5),
               dict(restart_interval=-1), dict(restart_interval=65536)):
        with pytest.raises(ValueError):
            jpeg.encode([img], encoder="host", **kw)
    for shape in ((0, 8), (8, 0), (65536, 1), (1, 65536)):
        with pytest.raises(ValueError):
            K.jpeg_enc_images([shape])
    with pytest.raises(ValueError, match="grey"):
        jpeg.encode([np.zeros((8, 8), dtype=np.uint8)], encoder="host")
    with pytest.raises(ValueError, match="CMYK"):
        jpeg.encode([np.zeros((8, 8, 4), dtype=np.uint8)], encoder="host")
    with pytest.raises(ValueError):
        jpeg.encode([img], encoder="cpu")
    for option in ("optimize", "progressive", "arithmetic", "exif", "icc_profile", "comment"):
        with pytest.raises(ValueError, match="scope"):
            jpeg.write_jpeg("unused.jpg", img, encoder="host", **{option: True})
    # the library itself validates the descriptor and the pointers
    lib = shdr._lib.load()
    d = _desc(K, 8, 8, "420")
    for field, value in (("layout", 3), ("layout", -1), ("quality", 0), ("quality", 101), ("height", 0), ("width", 65536), ("restart", 65536)):
        bad = d.copy()
        bad[field] = value
        assert lib.shdr_jpeg_encode_blocks(K._hptr(bad), None) == -1
        assert lib.shdr_jpeg_encode_host(K._hptr(img), K._hptr(bad), K._hptr(np.zeros(4096, dtype=np.uint8)), 4096) == -1
    out = np.zeros(4096, dtype=np.uint8)
    coef = np.zeros((6, 64), dtype=np.int16)
    assert lib.shdr_jpeg_encode_host(None, K._hptr(d), K._hptr(out), 4096) == -5
    assert lib.shdr_jpeg_encode_host(K._hptr(img), None, K._hptr(out), 4096) == -5
    assert lib.shdr_jpeg_encode_host(K._hptr(img), K._hptr(d), None, 4096) == -5
    assert lib.shdr_jpeg_encode_transform_host(None, K._hptr(d), K._hptr(coef), 6) == -5
    assert lib.shdr_jpeg_encode_transform_host(K._hptr(img), K._hptr(d), None, 6) == -5
    assert lib.shdr_jpeg_encode_transform_host(K._hptr(img), K._hptr(d), K._hptr(coef), 5) == -1
    assert lib.shdr_jpeg_encode_entropy_host(None, 6, K._hptr(d), K._hptr(out), 4096) == -5
    assert lib.shdr_jpeg_encode_entropy_host(K._hptr(coef), 6, K._hptr(d), None, 4096) == -5
    assert lib.shdr_jpeg_encode_header_host(K._hptr(d), None) == -5
    assert lib.shdr_jpeg_encode_batch_sizes(None, 1, None, None, None) == -5
    assert lib.shdr_jpeg_encode_batch_sizes(K._hptr(d), 0, None, None, None) == -1
    assert b"jpeg_encode" in lib.shdr_last_error()


def test_short_capacity_fails_and_leaves_the_guard(shdr):
    K = shdr._ops
    img = R.content("noise", 24, 40, seed=3)
    d = _desc(K, 24, 40, "420", 90, 2)
    whole = K.jpeg_encode_host(img, d)
    coef = K.jpeg_encode_transform_host(img, d)
    scan = K.jpeg_encode_entropy_host(coef, d)
    got, guard = K.jpeg_encode_host(img, d, capacity=len(whole), guard=64)
    assert got == whole and (guard == K.JPEG_ENC_GUARD).all()
    got, guard = K.jpeg_encode_entropy_host(coef, d, capacity=len(scan), guard=64)
    assert got == scan and (guard == K.JPEG_ENC_GUARD).all()
    for fn, arg, full in ((K.jpeg_encode_host, img, len(whole)), (K.jpeg_encode_entropy_host, coef, len(scan))):
        for cap in (full - 1, full // 2, 1, 0):
            with pytest.raises(ValueError, match="does not fit") as exc:
                fn(arg, d, capacity=cap, guard=64)
            assert exc.value.guard.size == 64 and (exc.value.guard == K.JPEG_ENC_GUARD).all(), cap
