"""The host twin of the device inflate (shdr_inflate_host, csrc/inflate.h), through ctypes, judged by zlib: a stream is accepted exactly
where exr.read_payload's rule accepts it (deflate_synth.accepts), and then byte for byte zlib's output.  No tolerances."""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_synth as S
import exr_ref as R
from test_deflate_host import CHUNKS

VALID = S.valid_cases()
INVALID = S.invalid_cases()


def contents():
    """zeros, a period-3 pattern, random bytes and what ZIP really deflates: a predicted block of 16 HALF scanlines, ramps with noise"""
    rng = np.random.default_rng(17)
    n = 6000
    ramp = (np.linspace(0.1, 4.0, 3 * 16 * 64).reshape(16, 3, 64) * (1 + 0.01 * rng.standard_normal((16, 3, 64)))).astype("<f2")
    return {"zeros": bytes(n), "period3": (b"\x01\x80\xfe" * n)[:n], "random": rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
            "exr_half_ramp": R.predict(ramp.tobytes())}


def zlib_streams():
    """[(name, stream, want)] of zlib's own compressor: levels 0 (70000 bytes: more than one stored block), 1, 6, 9; every strategy;
    wbits 9 .. 15; four kinds of content"""
    out = []
    strategies = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman_only": zlib.Z_HUFFMAN_ONLY,
                  "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}

    def add(name, data, level, wbits, strategy):
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
        out.append((name, c.compress(data) + c.flush(), len(data)))

    for cname, data in contents().items():
        for level in (0, 1, 6, 9):
            for sname, strategy in strategies.items():
                add("%s_l%d_%s_w15" % (cname, level, sname), data, level, 15, strategy)
        for wbits in range(9, 15):
            for level in (1, 6, 9):
                add("%s_l%d_default_w%d" % (cname, level, wbits), data, level, wbits, zlib.Z_DEFAULT_STRATEGY)
    big = np.random.default_rng(18).integers(0, 256, 70000, dtype=np.uint8).tobytes()
    add("random_70000_l0", big, 0, 15, zlib.Z_DEFAULT_STRATEGY)
    return out


ZLIB = zlib_streams()


def first_block_type(stream):
    return (stream[2] >> 1) & 3


def check(K, stream, want):
    """K.inflate_host against the oracle; returns the status"""
    got, status = K.inflate_host(stream, want)
    assert len(got) <= want
    if S.accepts(stream, want):
        assert status == 0 and got == zlib.decompress(stream)
    else:
        assert status != 0
    return status


def test_the_corpus_holds_every_block_type():
    """so that no block type can silently go missing from what the host and the device tests run"""
    streams = [s for _, s, _ in VALID + ZLIB]
    assert {first_block_type(s) for s in streams} == {0, 1, 2}
    by_name = {n: s for n, s, _ in ZLIB}
    assert first_block_type(by_name["exr_half_ramp_l6_fixed_w15"]) == 1
    assert first_block_type(by_name["random_70000_l0"]) == 0 and len(by_name["random_70000_l0"]) == 70016
    assert first_block_type(by_name["exr_half_ramp_l6_default_w15"]) == 2


@pytest.mark.parametrize("name,stream,want", VALID, ids=[c[0] for c in VALID])
def test_synthetic_valid(shdr, name, stream, want):
    assert check(shdr._ops, stream, want) == 0


@pytest.mark.parametrize("name,stream,want", INVALID, ids=[c[0] for c in INVALID])
def test_synthetic_invalid(shdr, name, stream, want):
    assert check(shdr._ops, stream, want) != 0


def test_failure_classes_have_their_own_codes(shdr):
    K = shdr._ops
    status = {name: K.inflate_host(stream, want)[1] for name, stream, want in INVALID}
    expect = {"empty_input": 1, "truncated_in_zlib_header": 1, "truncated_in_a_code": 1, "truncated_in_adler_2": 1, "cm_7": 2, "cinfo_8": 2,
              "header_check": 2, "fdict": 3, "block_type_3": 4, "stored_nlen": 5, "hlit_287": 6, "hdist_31": 6,
              "code_length_code_oversubscribed": 7, "code_length_code_incomplete": 7, "repeat_16_first": 8, "run_overflows": 9,
              "no_end_of_block": 10, "literal_set_oversubscribed": 11, "literal_set_incomplete": 11, "distance_set_oversubscribed": 12,
              "distance_set_incomplete": 12, "unassigned_literal_code": 13, "literal_symbol_286": 13, "literal_symbol_287": 13,
              "unassigned_distance_code": 14, "match_without_distance_codes": 14, "distance_symbol_30": 14, "distance_symbol_31": 14,
              "distance_before_first_byte": 15, "distance_too_far_back": 15, "output_one_longer_than_slot": 16,
              "output_one_shorter_than_slot": 17, "wrong_adler": 18}
    assert {n: status[n] for n in expect} == expect
    assert all(K.inflate_reason(s) != "ok" for s in status.values()) and K.inflate_reason(0) == "ok"


def test_zlib_streams(shdr):
    for name, stream, want in ZLIB:
        assert check(shdr._ops, stream, want) == 0, name


@pytest.mark.parametrize("name", sorted(CHUNKS))
def test_streams_of_the_projects_encoder(shdr, name):
    K = shdr._ops
    stream = K.deflate_huffman_host(CHUNKS[name])
    got, status = K.inflate_host(stream, len(CHUNKS[name]))
    assert status == 0 and got == CHUNKS[name]
    assert K.inflate_host(stream, len(CHUNKS[name]) - 1)[1] == 16 and K.inflate_host(stream, len(CHUNKS[name]) + 1)[1] == 17


def test_every_bit_flip_and_truncation_of_the_small_streams(shdr):
    """the exhaustive mutation sweep (host only): accepted exactly where zlib accepts, never more bytes than the slot"""
    K = shdr._ops
    runs = 0
    for name, stream, want in VALID + INVALID:
        if len(stream) > 120:
            continue
        for cut in range(len(stream)):
            check(K, stream[:cut], want)
        for bit in range(8 * len(stream)):
            m = bytearray(stream)
            m[bit >> 3] ^= 1 << (bit & 7)
            check(K, bytes(m), want)
        runs += 9 * len(stream)
    assert runs > 5000


def test_nothing_is_written_beyond_the_capacity(shdr):
    lib = shdr._lib.load()
    for name, stream, want in VALID + INVALID:
        if want > 70000:
            continue
        src = np.frombuffer(stream, dtype=np.uint8)
        for capacity in sorted({0, want // 2, max(want - 1, 0), want}):
            out = np.full(capacity + 64, 0xC3, dtype=np.uint8)
            st = ctypes.c_int(-1)
            n = lib.shdr_inflate_host(ctypes.c_void_p(src.ctypes.data if src.size else None), src.size, ctypes.c_void_p(out.ctypes.data),
                                      capacity, ctypes.byref(st))
            assert 0 <= n <= capacity and np.all(out[capacity:] == 0xC3), (name, capacity)
            assert (st.value == 0) == (S.accepts(stream, capacity))


def test_bad_arguments(shdr):
    lib = shdr._lib.load()
    st = ctypes.c_int(0)
    buf = np.zeros(8, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert lib.shdr_inflate_host(p, -1, p, 8, ctypes.byref(st)) == -1 and b"inflate_host" in lib.shdr_last_error()
    assert lib.shdr_inflate_host(None, 8, p, 8, ctypes.byref(st)) == -1
    assert lib.shdr_inflate_host(p, 8, None, 8, ctypes.byref(st)) == -1
    assert lib.shdr_inflate_host(p, 8, p, (1 << 30) + 1, ctypes.byref(st)) == -1
    assert lib.shdr_inflate_host(p, 8, p, 8, None) == -1
