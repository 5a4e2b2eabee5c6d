"""The host PIZ decoder (libshdr's shdr_piz_decode_host, csrc/piz.h: the rules the kernels run too) against piz_ref, the tests' own
PIZ codec: known answers, a chunk assembled by hand, the shared case matrix, every status, and every single-bit flip and truncation of
two small chunks.  Decoding is lossless: every comparison is equality of bytes.  No GPU."""
import importlib
import struct

import numpy as np
import pytest

import piz_cases
import piz_ref

K = importlib.import_module("singlehdr-tf2_amd._ops")


def ref_decode(data, width, rows, words):
    try:
        return piz_ref.decode_chunk(data, width, rows, words)
    except piz_ref.PizError:
        return None


def u16(values):
    return np.asarray(values, dtype="<u2").tobytes()


# ---- known answers --------------------------------------------------------------------------------------------------------
def test_known_wavelet_pairs_ref():
    assert tuple(int(v) for v in piz_ref.dec14(3, 3)) == (5, 2)
    assert tuple(int(v) for v in piz_ref.dec16(0x1000, 0)) == (0x9000, 0x1000)


def test_known_canonical_codes_ref():
    codes = piz_ref.canonical_codes({0: 2, 2: 3, 3: 3, 4: 1})
    assert codes == {0: 0b01, 2: 0b000, 3: 0b001, 4: 0b1}


# width 2, rows 3, one HALF channel.  Code lengths [2, 0, 3, 3, 1, 0] of symbols 0 .. 5 (no run code: symbol 5 has none): the table is
# 000010 000000 000011 000011 000001 000000 = 08 00 C3 04 00; the values 4 4 4 4 3 3 are 1 1 1 1 001 001 = F2 40, 10 bits.
HAND = (bytes([0x00, 0x00, 0x01, 0x00, 0xFF, 0xFF])                   # minNonZero 0, maxNonZero 1, values 0 .. 15 present
        + struct.pack("<i", 27)
        + struct.pack("<IIIII", 0, 5, 5, 10, 0) + bytes([0x08, 0x00, 0xC3, 0x04, 0x00]) + bytes([0xF2, 0x40]))
# the 2 x 2 block: dec14(4, 4) = (6, 2) twice, then dec14(6, 6) = (9, 3) and dec14(2, 2) = (3, 1); the left-over row: dec14(3, 3) = (5, 2)
HAND_OUT = u16([9, 3, 3, 1, 5, 2])


def test_hand_assembled_chunk():
    out, st = K.piz_decode_host(HAND, 2, 3, [1])
    assert (st, out) == (0, HAND_OUT)
    assert piz_ref.decode_chunk(HAND, 2, 3, [1]) == HAND_OUT


def test_known_dec16_through_the_decoder():
    # a full bitmap: the LUT is the identity and the 16-bit pair is used; the left-over row of a 2 x 3 plane is dec16(0x1000, 0)
    block = piz_ref.huf_encode([0, 0, 0, 0, 0x1000, 0], runs=False)
    chunk = piz_cases.assemble(block, range(65536))
    out, st = K.piz_decode_host(chunk, 2, 3, [1])
    assert st == 0
    assert out[8:] == u16([0x9000, 0x1000])
    assert out == piz_ref.decode_chunk(chunk, 2, 3, [1])


def test_lut_from_bitmap():
    # 7 x 1: no wavelet level, so the output is the LUT of the values 0 .. 6; value 0 is present whatever the bitmap says
    present = (3, 8, 9, 300, 65535)
    chunk = piz_cases.assemble(piz_ref.huf_encode(list(range(7)), runs=False), present)
    out, st = K.piz_decode_host(chunk, 7, 1, [1])
    assert (st, out) == (0, u16([0, 3, 8, 9, 300, 65535, 0]))
    assert piz_ref.decode_chunk(chunk, 7, 1, [1]) == out


# ---- the reference itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mx", [100, 16383, 16384, 65535])
def test_ref_wavelet_round_trip_and_forms(mx):
    rng = np.random.default_rng(mx)
    for ny, nx in ((1, 1), (1, 9), (5, 2), (3, 3), (17, 33), (32, 100), (31, 7), (32, 32), (6, 65)):
        plane = rng.integers(0, 1 << 16, (ny, nx))
        coded = piz_ref.wav_encode(plane, mx)
        assert np.array_equal(piz_ref.wav_decode(coded, mx), plane)
        if nx * ny <= 600:
            assert np.array_equal(piz_ref.wav_decode_loops(coded, mx), plane)


@pytest.mark.parametrize("ny", [1, 2, 3, 5, 8, 13, 17, 31, 32])
def test_full_plane_wavelet_equals_strip_form(ny):
    # aligned strips of P columns never touch each other at any level, the left-over column and row rules included
    rng = np.random.default_rng(ny)
    for nx in range(1, 101):
        plane = rng.integers(0, 1 << 16, (ny, nx))
        for mx in (1000, 65535):
            assert np.array_equal(piz_ref.wav_decode_strips(plane, mx), piz_ref.wav_decode(plane, mx)), (ny, nx, mx)


def test_ref_huffman_round_trip_forced_paths():
    rng = np.random.default_rng(5)
    vals = [int(v) for v in np.repeat(rng.integers(0, 40, 60), rng.integers(1, 9, 60))]
    for kw in (dict(), dict(runs=False), dict(long_runs=False), dict(min_run=1)):
        assert piz_ref.huf_decode(piz_ref.huf_encode(vals, **kw), len(vals)) == vals


def test_ref_fast_encoder_writes_the_same_bytes():
    for c in piz_cases.cases()[::9]:
        if c.raw is not None and "noruns" not in c.name and "shorttable" not in c.name:
            assert piz_ref.encode_chunk(c.raw, c.width, c.rows, c.words, force16=c.name.startswith(("noise16", "ramp_forced16")), fast=True) == c.data, c.name


# ---- the host twin over the matrix ------------------------------------------------------------------------------------------------
def test_host_equals_ref_equals_source_over_the_matrix():
    for c in piz_cases.cases():
        out, st = K.piz_decode_host(c.data, c.width, c.rows, c.words)
        assert st == 0, (c.name, K.piz_reason(st))
        assert out == piz_ref.decode_chunk(c.data, c.width, c.rows, c.words), c.name
        if c.raw is not None:
            assert out == c.raw, c.name


def test_matrix_reaches_both_wavelet_pairs_long_codes_and_runs():
    names = [c.name for c in piz_cases.cases()]
    assert any(n.startswith("noise16") for n in names) and any(n.startswith("noise14") for n in names)
    assert "ladder58_short" in names and "ladder58_long" in names and "run_first_in_subsequence" in names


# ---- every status -----------------------------------------------------------------------------------------------------------------
def _block(im, iM, n_bits, table=b"", data=b""):
    return struct.pack("<IIIII", im, iM, len(table), n_bits, 0) + table + data


def _chunk(block, bitmap=b"\xff\xff", lo=0, hi=1):
    return struct.pack("<HH", lo, hi) + bitmap + struct.pack("<i", len(block)) + block


TABLE = bytes([0x08, 0x00, 0xC3, 0x04, 0x00])        # lengths [2, 0, 3, 3, 1, 0] of symbols 0 .. 5
RUN_TABLE = bytes([0x04, 0x10])                      # lengths [1, 1] of symbols 0 and 1 (the run code)
STATUS_CHUNKS = {
    1: [b"\0\0", struct.pack("<HH", 0, 1) + b"\xff\xff" + b"\x1b\0"],
    2: [struct.pack("<HH", 0, 8192) + b"\0" * 9000, struct.pack("<HH", 0, 100) + b"\0" * 50],
    3: [struct.pack("<HH", 0, 1) + b"\xff\xff" + struct.pack("<i", -1), struct.pack("<HH", 0, 1) + b"\xff\xff" + struct.pack("<i", 28) + b"\0" * 27],
    4: [_chunk(b""), _chunk(_block(0, 5, 0, TABLE, b"\xf2\x40"))],
    5: [_chunk(b"\0" * 19), _chunk(_block(65537, 65537, 10, TABLE)), _chunk(_block(0, 65537, 10, TABLE)), _chunk(_block(3, 2, 10, TABLE))],
    6: [_chunk(_block(0, 5, 10, TABLE[:4])), _chunk(_block(0, 300, 10, bytes([0xFC])))],
    7: [_chunk(_block(0, 5, 10, bytes([0x08, 0x0F, 0xC0, 0x00]))),        # 2, 0, then 63 -> a run of 6 + 0 zeros from symbol 2
        _chunk(_block(0, 5, 10, bytes([0x08, 0x00, 0xC3, 0x07, 0xB0])))],  # 2, 0, 3, 3, 1, then 59 -> two zeros from symbol 5
    8: [_chunk(_block(0, 2, 10, bytes([0x04, 0x10, 0x40]), b"\0\0"))],    # lengths 1, 1, 1
    9: [_chunk(_block(0, 5, 17, TABLE, b"\xf2\x40"))],
    10: [_chunk(_block(0, 5, 10, bytes([0x08, 0x00, 0xC3, 0x00, 0x00]), b"\xf2\x40"))],   # lengths 2, 0, 3, 3, 0, 0: nobody owns 1...
    11: [_chunk(_block(0, 5, 9, TABLE, b"\xf2\x40")),                     # the last 001 is cut
         _chunk(_block(0, 1, 6, RUN_TABLE, b"\x60\x40"))],                # 0, run with 4 of its 8 count bits
    12: [_chunk(_block(0, 1, 9, RUN_TABLE, b"\x81\x00"))],                # a run of 2 as the first token
    13: [_chunk(_block(0, 5, 10, TABLE, b"\xff\xc0")),                    # ten values
         _chunk(_block(0, 1, 10, RUN_TABLE, b"\x41\x80"))],               # 0, then a run of 6: seven values
    14: [_chunk(_block(0, 5, 4, TABLE, b"\xf0")),                         # four values
         _chunk(_block(0, 1, 10, RUN_TABLE, b"\x40\x00"))],               # 0, then a run of 0: writes nothing
}


@pytest.mark.parametrize("status", sorted(STATUS_CHUNKS))
def test_every_status_is_reached(status):
    for chunk in STATUS_CHUNKS[status]:
        out, st = K.piz_decode_host(chunk, 2, 3, [1])
        assert (st, out) == (status, b""), (K.piz_reason(st), chunk.hex())
        assert ref_decode(chunk, 2, 3, [1]) is None


def test_statuses_are_named():
    assert len(K.PIZ_REASONS) == 17 and K.piz_reason(0) == "ok" and K.piz_reason(99) == "status 99"
    assert sorted(STATUS_CHUNKS) == list(range(1, 15))                 # 15 and 16 belong to the batch call (tests/test_gpu_piz.py)


def test_bad_arguments_are_errors_not_statuses():
    with pytest.raises(ValueError):
        K.piz_decode_host(HAND, 2, 33, [1])
    with pytest.raises(ValueError):
        K.piz_decode_host(HAND, 2, 3, [3])
    with pytest.raises(ValueError):
        K.piz_decode_host(HAND, 2, 3, [1], out=np.zeros(13, dtype=np.uint8))


# ---- every single-bit flip and every truncation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_every_bit_flip_and_truncation(which):
    c = piz_cases.small_cases()[which]
    want = 2 * c.width * c.rows * sum(c.words)
    good, _ = K.piz_decode_host(c.data, c.width, c.rows, c.words)
    assert good == piz_ref.decode_chunk(c.data, c.width, c.rows, c.words) and (c.raw is None or good == c.raw)
    accepted = 0
    for name, data in piz_cases.mutations(c.data):
        guard = np.full(want + 64, 0xA5, dtype=np.uint8)
        _, st = K.piz_decode_host(data, c.width, c.rows, c.words, out=guard[:want])
        assert 0 <= st < len(K.PIZ_REASONS), name
        assert (guard[want:] == 0xA5).all(), name                         # never a byte beyond the capacity
        ref = ref_decode(data, c.width, c.rows, c.words)
        assert (st == 0) == (ref is not None), (name, K.piz_reason(st))
        if st == 0:
            assert guard[:want].tobytes() == ref, name
            accepted += 1
        else:
            assert (guard[:want] == 0xA5).all(), name                     # a refused chunk leaves its slot untouched
    assert 0 < accepted < 9 * len(c.data)
