"""The host twin of the Radiance reader (shdr_rgbe_rle_decode_status, written from csrc/hdr_rle_dec.h, the rules the device kernels
run) against the independent NumPy reader tests/hdr_rle_dec_ref.py and against the law, shdr_rgbe_rle_decode: on every stream of
tests/hdr_rle_dec_cases.py the three accept or refuse together, with the same pixels and consumed count, the same failing scanline and
stop offset (twin and reference), and the message composed from (status, line) is the text the law leaves in shdr_last_error.  Byte
equality throughout.  Then the Python layer's GPU-free parts: read_scanlines, option validation, the message table."""
import ctypes
import importlib

import numpy as np
import pytest

import hdr_rle_dec_cases as C
import hdr_rle_dec_ref as REF

pkg = importlib.import_module("singlehdr-tf2_amd")
IO, K, LIB = pkg.hdr_io, pkg._ops, pkg._lib


def _law(data, w, h):
    """shdr_rgbe_rle_decode: (pixels, consumed) or the message"""
    lib = LIB.load()
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    n = lib.shdr_rgbe_rle_decode(ctypes.c_void_p(buf.ctypes.data if buf.size else out.ctypes.data), buf.size, w, h, ctypes.c_void_p(out.ctypes.data))
    if n < 0:
        return lib.shdr_last_error().decode()
    return out, n


def test_cases_cover_what_they_name():
    names = [c[0] for c in C.cases()]
    assert len(names) == len(set(names)) and len(names) > 500
    by = C.by_name()
    _, w, h, data = by["dense_514"]
    assert REF.count_candidates(data, w) == len(data) - 3 > 2 * h + 64
    for name in ("dense_514_flat", "dense_514_then_coded"):                               # over the cap, and files the host routine accepts
        _, w, h, data = by[name]
        assert REF.count_candidates(data, w) > 2 * h + 64 and isinstance(REF.decode(data, w, h)[0], np.ndarray)
    for h in (1, 3):
        assert REF.count_candidates(by["markers_at_cap_h%d" % h][3], 8) == 2 * h + 64
        assert REF.count_candidates(by["markers_over_cap_h%d" % h][3], 8) == 2 * h + 65
    assert REF.count_candidates(by["markers_over_cap_in_flat_lines"][3], 8) == 67
    for name in ("families_9x3", "families_257x65", "families_32767_0"):                 # decoded on the device, not handed back
        _, w, h, data = by[name]
        assert h <= REF.count_candidates(data, w) <= 2 * h + 64                             # (the families hold false markers too)
    statuses = {REF.decode(d, w, h)[0] for _, w, h, d in C.cases() if not isinstance(REF.decode(d, w, h)[0], np.ndarray)}
    assert statuses == {REF.TRUNCATED, REF.CORRUPT_RUN, REF.CORRUPT_LITERAL, REF.TRUNCATED_FLAT}


def test_twin_reference_and_law_agree_on_every_case():
    refused = 0
    for name, w, h, data in C.cases():
        want = REF.decode(data, w, h)
        pixels, status, line, consumed = K.rgbe_rle_decode_host(data, w, h)
        law = _law(data, w, h)
        if isinstance(want[0], np.ndarray):
            assert status == 0 and line == -1 and consumed == want[1], name
            assert np.array_equal(pixels, want[0]), name
            assert not isinstance(law, str) and law[1] == consumed and np.array_equal(law[0], pixels), name
            assert consumed <= len(data)
        else:
            refused += 1
            assert pixels is None and (status, line, consumed) == want, (name, (status, line, consumed), want)
            assert isinstance(law, str), name
            assert K.rgbe_dec_message(status, line) == law == REF.MESSAGES[status] % line, name
    assert refused > 300


def test_consumed_stops_short_of_trailing_bytes():
    by = C.by_name()
    w, h, data = C.small_coded()
    for name in ("trailing_garbage", "trailing_marker", "trailing_whole_line", "trailing_line_with_corrupt_run"):
        pixels, status, _, consumed = K.rgbe_rle_decode_host(by[name][3], w, h)
        assert status == 0 and consumed == len(data) < len(by[name][3])
        assert np.array_equal(pixels, IO.rle_decode(data, h, w))


def test_twin_refuses_bad_arguments():
    lib = LIB.load()
    out = np.zeros(64, dtype=np.uint8)
    st, ln, stop = ctypes.c_int(-7), ctypes.c_int(0), ctypes.c_int64(0)
    args = (ctypes.byref(st), ctypes.byref(ln), ctypes.byref(stop))
    p = ctypes.c_void_p(out.ctypes.data)
    assert lib.shdr_rgbe_rle_decode_status(None, 4, 1, 1, p, *args) == -1 and st.value == -7
    assert b"rgbe_rle_decode_status" in lib.shdr_last_error()
    assert lib.shdr_rgbe_rle_decode_status(p, 4, 0, 1, p, *args) == -1
    assert lib.shdr_rgbe_rle_decode_status(p, -1, 1, 1, p, *args) == -1
    assert lib.shdr_rgbe_rle_decode_status(p, 4, 1, 1, None, *args) == -1
    assert lib.shdr_rgbe_rle_decode_status(None, 0, 1, 1, p, *args) == -1 and st.value == REF.TRUNCATED_FLAT      # an empty file is a file
    with pytest.raises(ValueError):
        K.rgbe_rle_decode_host(b"", 0, 1)


def test_message_table():
    assert set(K.RGBE_DEC_REASONS) == {K.RGBE_DEC_TRUNCATED, K.RGBE_DEC_CORRUPT_RUN, K.RGBE_DEC_CORRUPT_LITERAL, K.RGBE_DEC_TRUNCATED_FLAT}
    assert (K.RGBE_DEC_OK, K.RGBE_DEC_TRUNCATED, K.RGBE_DEC_CORRUPT_RUN, K.RGBE_DEC_CORRUPT_LITERAL, K.RGBE_DEC_TRUNCATED_FLAT,
            K.RGBE_DEC_FALLBACK) == (REF.OK, REF.TRUNCATED, REF.CORRUPT_RUN, REF.CORRUPT_LITERAL, REF.TRUNCATED_FLAT, REF.FALLBACK)
    assert K.rgbe_dec_message(K.RGBE_DEC_TRUNCATED_FLAT, 12) == "rgbe_rle_decode: truncated data in flat scanline 12"
    for status in (K.RGBE_DEC_OK, K.RGBE_DEC_FALLBACK, 17):
        with pytest.raises(ValueError):
            K.rgbe_dec_message(status, 0)


def _files(tmp_path):
    rng = np.random.default_rng(0)
    paths = []
    for i, (h, w) in enumerate(((5, 9), (3, 7), (2, 300), (4, 128))):
        img = C.R.family_image(h, w, seed=i) if w >= 7 else rng.integers(0, 256, size=(h, w, 4)).astype(np.uint8)
        path = str(tmp_path / ("f%d.hdr" % i))
        IO.write_hdr(path, img)
        paths.append((path, img))
    return paths


def test_read_scanlines_and_twin_equal_read_rgbe(tmp_path):
    for path, img in _files(tmp_path):
        lines = IO.read_scanlines(path)
        assert (lines.height, lines.width, lines.path) == (img.shape[0], img.shape[1], path) and lines.shape == img.shape
        pixels, status, _, consumed = K.rgbe_rle_decode_host(lines.data, lines.width, lines.height)
        assert status == 0 and consumed == len(lines.data)
        assert np.array_equal(pixels, img) and np.array_equal(IO.read_rgbe(path), img) and np.array_equal(lines.decode(), img)
    assert [np.array_equal(a, img) for a, (_, img) in zip(IO.read_rgbe_batch([p for p, _ in _files(tmp_path)]), _files(tmp_path))] == [True] * 4


def test_host_refusals_carry_the_path(tmp_path):
    (path, _), (good, _) = _files(tmp_path)[:2]
    with open(path, "rb") as f:
        data = f.read()
    with open(path, "wb") as f:
        f.write(data[:-3])
    with pytest.raises(ValueError) as exc:
        IO.read_rgbe_batch([good, path], decoder="host")
    assert str(exc.value) == "%s: rgbe_rle_decode: truncated data in scanline 4" % path
    with pytest.raises(ValueError) as exc:
        IO.read_rgbe(path)
    assert str(exc.value).startswith(path + ": rgbe_rle_decode: ")
    with open(path, "wb") as f:
        f.write(b"\x76\x2f\x31\x01rest")
    with pytest.raises(ValueError, match="OpenEXR"):
        IO.read_scanlines(path)


def test_option_validation():
    for fn in (lambda: IO.read_rgbe("nowhere.hdr", decoder="gpu"), lambda: IO.read_rgbe_batch([], decoder="cuda"),
               lambda: IO.check_decoder_option("somebody", None)):
        with pytest.raises(ValueError, match="'host' or 'device'"):
            fn()
    assert IO.check_decoder_option("x", "host") == "host" and IO.check_decoder_option("x", "device") == "device"
    assert IO.read_rgbe_batch([], decoder="host") == [] and IO.rle_decode_device([]) == []
    with pytest.raises(ValueError, match="'host' or 'device'"):
        pkg.dataset.HDRDataset("nowhere", [], True, hdr_rle="both")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        pkg.hdr_real.HdrRealFolder("nowhere", hdr_rle="both")
