"""The host PIZ encoder (shdr_piz_encode_host, csrc/piz.h) against the independent encoder and decoder of tests/piz_ref.py: the same bytes
for every chunk of tests/piz_enc_cases.py, round trips through both decoders, the wavelet pairs' known answers, every argument error.
No GPU: only the library's host routines run."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import piz_enc_cases  # noqa: E402
import piz_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PKG = importlib.import_module("singlehdr-tf2_amd")
K = PKG._ops
LIB = PKG._lib

CHUNKS = piz_enc_cases.chunks()
IDS = [c.name for c in CHUNKS]


@pytest.fixture(scope="module")
def twin():
    """the host twin's bytes of every chunk, once"""
    return {c.name: K.piz_encode_host(c.raw, c.width, c.rows, c.words) for c in CHUNKS}


def test_the_named_chunks_are_there():
    names = set(IDS)
    assert {"zeros_9x5", "constant_33x17", "ordered_100x32", "shuffled_100x32", "stretches_65x32", "one_pixel"} <= names
    assert any(n.startswith("table_zeros_") for n in names)
    assert len(CHUNKS) >= 60
    ordered = next(c for c in CHUNKS if c.name == "ordered_100x32")
    assert np.unique(np.frombuffer(ordered.raw, dtype="<u2")).size == 19200 > 16384       # the 16-bit pair is certain


@pytest.mark.parametrize("c", CHUNKS, ids=IDS)
def test_bytes_equal_the_reference(c, twin):
    want = piz_ref.encode_chunk(c.raw, c.width, c.rows, c.words)
    assert twin[c.name] == want
    assert piz_ref.encode_chunk(c.raw, c.width, c.rows, c.words, fast=True) == want


@pytest.mark.parametrize("c", CHUNKS, ids=IDS)
def test_round_trip(c, twin):
    got, status = K.piz_decode_host(twin[c.name], c.width, c.rows, c.words)
    assert status == 0, K.piz_reason(status)
    assert got == c.raw
    assert piz_ref.decode_chunk(twin[c.name], c.width, c.rows, c.words) == c.raw


def test_coded_or_raw(twin):
    """one level up a chunk is stored as PIZ only where that is strictly smaller"""
    size = {c.name: (len(twin[c.name]), len(c.raw)) for c in CHUNKS}
    assert size["ordered_100x32"][0] < size["ordered_100x32"][1]
    assert size["shuffled_100x32"][0] >= size["shuffled_100x32"][1]
    assert size["one_pixel"][0] >= size["one_pixel"][1]
    assert twin["zeros_9x5"][:4] == bytes([0xFF, 0x1F, 0, 0])                 # an empty bitmap: 8191 / 0


PAIRS14 = [((0, 0), (0, 0)), ((5, 3), (4, 2)), ((3, 5), (4, 0xFFFE)), ((100, 0), (50, 100)), ((7, 0), (3, 7)), ((0, 7), (3, 0xFFF9)),
           ((0x3FFF, 0), (0x1FFF, 0x3FFF)), ((0, 0x3FFF), (0x1FFF, 0xC001)), ((0x1FFF, 0x2000), (0x1FFF, 0xFFFF))]
PAIRS16 = [((0, 0), (0x4000, 0x8000)), ((5, 3), (0x4004, 0x8002)), ((3, 5), (0x4004, 0x7FFE)), ((0xFFFF, 0), (0x3FFF, 0x7FFF)),
           ((0, 0xFFFF), (0x3FFF, 0x8001)), ((0x8000, 0x8000), (0xC000, 0x8000)), ((0x1234, 0xABCD), (0x1F00, 0xE667))]
ENC14, ENC16, DEC14, DEC16 = 0, 1, 2, 3                                   # shdr_piz_wavelet_pair's `which`


def _pair(which, a, b):
    out = (ctypes.c_uint16 * 2)()
    assert LIB.load().shdr_piz_wavelet_pair(which, a, b, out) == 0
    return out[0], out[1]


def test_wavelet_pairs_known_answers():
    for (a, b), (l, h) in PAIRS14:
        assert _pair(ENC14, a, b) == (l, h), (a, b)
        assert _pair(DEC14, l, h) == (a, b), (l, h)
    for (a, b), (l, h) in PAIRS16:
        assert _pair(ENC16, a, b) == (l, h), (a, b)
        assert _pair(DEC16, l, h) == (a, b), (l, h)


def test_wavelet_pairs_round_trip():
    """all pairs of a 256-value subset, both pairs, against piz_ref's and back through the decoder's"""
    rng = np.random.default_rng(3)
    edge = [0, 1, 2, 0x3FFF, 0x4000, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF]
    vals = np.concatenate([edge, rng.choice(np.setdiff1d(np.arange(65536), edge), 256 - len(edge), replace=False)])
    assert np.unique(vals).size == 256
    a, b = [x.reshape(-1) for x in np.meshgrid(vals, vals, indexing="ij")]
    for enc, dec, ref in ((ENC14, DEC14, piz_ref.enc14), (ENC16, DEC16, piz_ref.enc16)):
        rl, rh = ref(a, b)
        for i in range(a.size):
            l, h = _pair(enc, int(a[i]), int(b[i]))
            assert (l, h) == (int(rl[i]), int(rh[i]))
            assert _pair(dec, l, h) == (int(a[i]), int(b[i]))


def _encode_rc(raw, n, width, rows, words, capacity, null=None):
    lib = LIB.load()
    src = np.frombuffer(raw, dtype=np.uint8)
    w = np.ascontiguousarray(words, dtype=np.int32)
    out = np.full(max(capacity, 1) + 16, 0xA5, dtype=np.uint8)
    written = ctypes.c_int64(-7)
    rc = lib.shdr_piz_encode_host(None if null == "raw" else src.ctypes.data, n, width, rows, None if null == "words" else w.ctypes.data,
                                  len(words), None if null == "dst" else out.ctypes.data, capacity,
                                  None if null == "written" else ctypes.byref(written))
    return rc, written.value, out


def test_argument_errors():
    lib = LIB.load()
    assert lib.shdr_piz_wavelet_pair(4, 0, 0, (ctypes.c_uint16 * 2)()) < 0 and lib.shdr_piz_wavelet_pair(0, 0, 0, None) < 0
    raw = np.arange(3 * 4 * 3, dtype="<u2").tobytes()
    good = (raw, len(raw), 4, 3, [1, 1, 1])
    need = len(K.piz_encode_host(raw, 4, 3, [1, 1, 1]))
    rc, written, out = _encode_rc(*good, need)
    assert rc == 0 and written == need and (out[need:] == 0xA5).all()
    for what, args in (("rows 0", (raw, len(raw), 4, 0, [1, 1, 1])), ("rows 33", (raw, len(raw), 4, 33, [1, 1, 1])),
                       ("no channel", (raw, len(raw), 4, 3, [])), ("65 channels", (raw, len(raw), 4, 3, [1] * 65)),
                       ("0 words", (raw, len(raw), 4, 3, [1, 0, 1])), ("3 words", (raw, len(raw), 4, 3, [1, 3, 1])),
                       ("size", (raw, len(raw) - 2, 4, 3, [1, 1, 1])), ("size", (raw, len(raw), 5, 3, [1, 1, 1])),
                       ("width 0", (raw, 0, 0, 3, [1, 1, 1]))):
        rc, written, out = _encode_rc(*args, 1 << 16)
        assert rc < 0 and written == -7 and (out == 0xA5).all(), what
        assert b"piz_encode_host" in lib.shdr_last_error()
    rc, written, out = _encode_rc(*good, need - 1)                       # too small a capacity: nothing is written
    assert rc < 0 and written == -7 and (out == 0xA5).all()
    for null in ("raw", "words", "dst", "written"):
        assert _encode_rc(*good, need, null=null)[0] < 0
    with pytest.raises(ValueError):
        K.piz_encode_host(raw, 4, 33, [1, 1, 1])
    with pytest.raises(ValueError):
        K.piz_encode_host(raw[:-2], 4, 3, [1, 1, 1])
    words = np.array([1, 1, 1], dtype=np.int32)
    assert lib.shdr_piz_encode_bound(4, 3, words.ctypes.data, 3) >= need
    assert lib.shdr_piz_encode_bound(4, 0, words.ctypes.data, 3) == -1


def test_bound_holds():
    lib = LIB.load()
    for c in CHUNKS:
        words = np.ascontiguousarray(c.words, dtype=np.int32)
        assert len(K.piz_encode_host(c.raw, c.width, c.rows, c.words)) <= lib.shdr_piz_encode_bound(c.width, c.rows, words.ctypes.data, words.size)
