"""CPU tests of the PNG writer: libshdr's host twin (K.png_filter_host, K.png_encode_host, csrc/png.h) against the NumPy restatement
of the rules (png_ref.py), against zlib's checksums and inflate, and against PIL's reader.  No kernel is launched here."""
import zlib

import numpy as np
import pytest

import png_ref as R

FILTER_CASES = R.filter_cases()
FILE_CASES = R.file_cases()


def test_case_list_reaches_every_filter_type_and_every_paeth_tie():
    """a condition on the inputs, asserted on the reference: each of the five types is chosen by at least one row"""
    chosen = set()
    for img in FILTER_CASES.values():
        chosen.update(int(t) for t in R.row_types(img))
    assert chosen == {0, 1, 2, 3, 4}
    assert set(R.paeth_tie_cases()) == {"pa=pb", "pb=pc", "pa=pc"}
    for name in ("zero_c1", "zero_c3", "zero_c4"):
        assert not R.row_types(FILTER_CASES[name]).any()                     # every row ties: type 0


@pytest.mark.parametrize("name", sorted(FILTER_CASES))
def test_filtered_stream_is_the_references(shdr, name):
    K = shdr._ops
    img = FILTER_CASES[name]
    assert K.png_filter_host(img) == R.filtered_stream(img), name
    for f in R.FILTERS:
        assert K.png_filter_host(img, f) == R.filtered_stream(img, f), (name, f)


def test_paeth_ties_follow_the_specification(shdr):
    K = shdr._ops
    for name, img in R.paeth_tie_cases().items():
        a, b, c, x = int(img[1, 0]), int(img[0, 1]), int(img[0, 0]), int(img[1, 1])
        want = {"pa=pb": a, "pb=pc": b, "pa=pc": a}[name]                    # a before b before c
        got = K.png_filter_host(img, "paeth")
        assert got[-1] == (x - want) & 255, name
        assert got == R.filtered_stream(img, "paeth")


@pytest.mark.parametrize("deflate", ["lz", "huffman"])
@pytest.mark.parametrize("name", sorted(FILE_CASES))
def test_whole_files(shdr, name, deflate):
    K = shdr._ops
    img, f = FILE_CASES[name]
    data = K.png_encode_host(img, f, deflate)
    idat = R.check_file(data, img, f)
    kinds = R.segment_kinds(idat)
    if name == "noise_stored":
        assert kinds == ["stored"] * 3
    if name == "coded_then_stored":
        assert kinds == ["coded", "stored"]
    if name == "long_row":
        assert len(idat) == 4 and "coded" in kinds
    if name in ("stream_65520", "stream_65519"):
        assert len(idat) == 1
    if name in ("stream_65521", "stream_131040"):
        assert len(idat) == 2
    assert K.png_encode_host(img, f, deflate, capacity=len(data)) == data    # exactly the size is enough


def test_filter_cases_as_files(shdr):
    K = shdr._ops
    for name, img in FILTER_CASES.items():
        R.check_file(K.png_encode_host(img), img)


def test_grey_without_a_channel_axis(shdr):
    K = shdr._ops
    img = R.noise(6, 9, 1, seed=3)
    assert K.png_encode_host(img[:, :, 0]) == K.png_encode_host(img)
    assert shdr.png.encode([img[:, :, 0], R.noise(3, 4, 4)], encoder="host")[0] == K.png_encode_host(img)


def test_crc32_is_zlibs(shdr):
    K = shdr._ops
    rng = np.random.default_rng(1)
    for n in (0, 1, 3, 4, 255, 256, 70001):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert K.crc32(b) == zlib.crc32(b)
        assert K.crc32(b[n // 2:], K.crc32(b[:n // 2])) == zlib.crc32(b)


def test_refusals(shdr):
    K = shdr._ops
    with pytest.raises(ValueError, match="C = 1"):
        K.png_encode_host(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(TypeError, match="uint8"):
        K.png_encode_host(np.zeros((4, 4, 3), np.uint16))
    with pytest.raises(TypeError, match="uint8"):
        K.png_filter_host(np.zeros((4, 4, 3), np.float32))
    for shape in ((0, 4, 3), (4, 0, 3)):
        with pytest.raises(ValueError, match="no pixels"):
            K.png_encode_host(np.zeros(shape, np.uint8))
    img = R.noise(5, 6, 3)
    size = len(K.png_encode_host(img))
    with pytest.raises(ValueError, match="too small"):
        K.png_encode_host(img, capacity=size - 1)
    with pytest.raises(ValueError, match="filter"):
        K.png_encode_host(img, filter="best")
    with pytest.raises(ValueError, match="deflate"):
        K.png_encode_host(img, deflate="zlib")
    with pytest.raises(ValueError, match="encoder"):
        shdr.png.encode([img], encoder="pil")
    # the library's own checks, behind the Python ones
    lib = shdr._lib.load()
    out = np.zeros(1024, np.uint8)
    px = np.zeros(64, np.uint8)
    for h, w, c in ((4, 4, 2), (0, 4, 3), (4, 0, 1), (4, 4, 0)):
        assert lib.shdr_png_encode_host(px.ctypes.data, h, w, c, 5, 1, out.ctypes.data, out.size) < 0
        assert lib.shdr_png_filter_host(px.ctypes.data, h, w, c, 5, out.ctypes.data, out.size) < 0
    assert lib.shdr_png_encode_host(px.ctypes.data, 4, 4, 3, 6, 1, out.ctypes.data, out.size) < 0
    assert lib.shdr_png_encode_host(px.ctypes.data, 4, 4, 3, 5, 2, out.ctypes.data, out.size) < 0
    assert lib.shdr_png_filter_host(px.ctypes.data, 4, 4, 3, 5, out.ctypes.data, 51) < 0
    assert "too small" in lib.shdr_last_error().decode()
