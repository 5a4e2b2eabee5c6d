"""The host routine of the LZ77 zlib encoder (shdr_deflate_lz_host / shdr_deflate_lz_parse_host, csrc/deflate_lz.h), through ctypes:
zlib's own inflate is the judge of the streams, the tokens are checked one by one, the code lengths and the header fields are read
back from the stream's bits, and the sizes are held against the Huffman-only encoder's on the content of tools/exr_write_bench.py."""
import hashlib
import zlib

import numpy as np
import pytest

from deflate_lz_cases import CASES, bench_content, distance_code, length_code, predicted_chunks
from test_deflate_host import CHUNKS, bits_of, value

NAMES = sorted(CASES)

# sha256 of shdr_deflate_huffman_host's stream for CHUNKS, from the build before build_lengths became a template
HUFFMAN_ONLY_SHA256 = {
    "all_256_values": "2c39330372eb76b78afd662c46b564c8858098643c1db684a2a5bc6b52424012",
    "ff_70000": "90afaaa3e5a93d0df193087edc7cb3288d1f3f942bdfc6e1f6201bf6d8ba070c",
    "fibonacci": "79e195bc71c6abfc93578f123c57522498eb0d1580c9000c657c58eab3755701",
    "len1": "3d921ddc200c09a185956f6ca6121b84ff4d0fa39c17bb75845dde96921e95b1",
    "len2": "6efb5f3ca934fd2e66eedcaf67b53f4a7eaf8e9405aa7b6fcdaf464fce222201",
    "len255": "79f879befaa6ce922a3c386eb656964efac2bc67da2c72c1593230fce3fae62d",
    "len256": "f08ca85ae9fe699aee6676712586cd857dfe98256366ed8565071b51144f69cd",
    "len257": "72cbcb9d1f73cdfdb5df145d1994f69f768f3c6095a1b7859211cbbe628dca3d",
    "len3": "33585b2acc051fffd5a5c38caa75e351a99ddc0a69176ac45d9a04ed5e2ca68e",
    "noisy_ramp": "447c8d4a80a28b1a8d2a6a7f9533faed2fb9119a2268c1191e2b75ab9a3a8ba0",
    "one_byte_repeated": "280709fafa05b15d47152760ce1c76765e00071b1827640cde56affa5d55ab87",
    "powers_of_two": "9f06e5ee780ee6692ce352ece7ccece75624268daa4e9d808bfb17778ef9ec3f",
}


@pytest.fixture(scope="module")
def streams(shdr):
    return {k: shdr._ops.deflate_lz_host(CASES[k]) for k in NAMES}


@pytest.fixture(scope="module")
def parses(shdr):
    return {k: shdr._ops.deflate_lz_parse_host(CASES[k]) for k in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_stream_inflates_to_the_chunk(shdr, streams, name):
    chunk, stream = CASES[name], streams[name]
    assert zlib.decompress(stream) == chunk
    d = zlib.decompressobj()
    assert d.decompress(stream) == chunk and d.eof and d.unused_data == b""
    assert shdr._ops.inflate_host(stream, len(chunk)) == (chunk, 0)
    assert stream[:2] == b"\x78\x01" and stream[-4:] == zlib.adler32(chunk).to_bytes(4, "big")


@pytest.mark.parametrize("name", NAMES)
def test_tokens_tile_and_rebuild_the_chunk(parses, name):
    chunk, at, out = CASES[name], 0, bytearray()
    for pos, length, dist in parses[name]:
        assert pos == at                                        # a token starts where the previous one ended
        if dist == 0:
            assert length == 1
            out.append(chunk[pos])
        else:
            assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= pos and pos + length <= len(chunk)
            assert not (length == 3 and dist > 4096)
            for _ in range(length):
                out.append(out[-dist])
        at += length
    assert at == len(chunk) and bytes(out) == chunk


def test_every_length_and_distance_code_occurs(parses):
    """no branch of the symbol writer is left unrun: all 29 length codes and all 30 distance codes, at both ends of their ranges"""
    lengths = {n for k in NAMES for _, n, d in parses[k] if d}
    dists = {d for k in NAMES for _, n, d in parses[k] if d}
    assert {length_code(n) for n in lengths} == set(range(29))
    assert {distance_code(d) for d in dists} == set(range(30))
    from deflate_lz_cases import boundary_distances, boundary_lengths
    assert set(boundary_lengths()) <= lengths and set(boundary_distances()) <= dists
    assert max(dists) == 32768 and max(lengths) == 258


def test_aimed_cases_parse_as_meant(parses):
    assert all(d == 0 for _, _, d in parses["no_match_at_all"]) and len(parses["no_match_at_all"]) == 256
    assert parses["one_distance_code"] == [(0, 1, 0), (1, 258, 1), (259, 41, 1)]
    assert parses["run_259"] == [(0, 1, 0), (1, 258, 1)] and parses["run_260"] == [(0, 1, 0), (1, 258, 1), (259, 1, 0)]
    assert parses["match_ends_the_chunk"][-1] == (120, 20, 120)
    assert parses["distance_32768"][-1] == (32768, 40, 32768)
    tail = [t for t in parses["distance_32769"] if t[0] >= 32769]
    assert all(d != 32769 and n < 40 for _, n, d in tail)                     # position 0 is out of reach: the block is not matched


def header(stream):
    """(HLIT, HDIST, HCLEN, the 19 code-length-code lengths, the 316 code lengths) read from the bits"""
    f = bits_of(stream, 16, 33)
    assert f[0] == 1 and value(f[1:3]) == 2                    # BFINAL, BTYPE: dynamic Huffman
    cl = bits_of(stream, 33, 33 + 57)
    body = bits_of(stream, 90, 90 + 4 * 316)                   # each length is the 4-bit code L, most significant bit first
    lens = [int("".join(map(str, body[4 * i:4 * i + 4])), 2) for i in range(316)]
    return value(f[3:8]), value(f[8:13]), value(f[13:17]), [value(cl[3 * i:3 * i + 3]) for i in range(19)], np.array(lens)


@pytest.mark.parametrize("name", NAMES)
def test_header_fields_and_both_codes(streams, parses, name):
    hlit, hdist, hclen, cl, lens = header(streams[name])
    assert (hlit, hdist, hclen) == (29, 29, 15)                 # 286 and 30 codes, all 19 code-length codes
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    assert cl == [4 if s <= 15 else 0 for s in order]
    lit_used, dist_used = np.zeros(286, bool), np.zeros(30, bool)
    lit_used[256] = True
    for pos, n, d in parses[name]:
        if d:
            lit_used[257 + length_code(n)] = dist_used[distance_code(d)] = True
        else:
            lit_used[CASES[name][pos]] = True
    lit, dist = lens[:286], lens[286:]
    assert np.all(lit[~lit_used] == 0) and np.all(lit[lit_used] >= 1) and lit.max() <= 15
    assert int((1 << (15 - lit[lit_used])).sum()) == 1 << 15                  # complete: a literal and end-of-block at the least
    assert np.all(dist[~dist_used] == 0) and dist.max() <= 15
    if dist_used.sum() == 1:
        assert dist[dist_used].tolist() == [1]                               # the one incomplete set zlib accepts
    elif dist_used.sum() >= 2:
        assert np.all(dist[dist_used] >= 1) and int((1 << (15 - dist[dist_used])).sum()) == 1 << 15


def test_the_three_forms_of_the_distance_code_occur(streams):
    used = {k: int((header(streams[k])[4][286:] > 0).sum()) for k in NAMES}
    assert used["no_match_at_all"] == 0 and used["one_distance_code"] == 1 and used["noisy_ramp"] >= 2


def test_white_noise_is_reported_as_not_smaller(streams):
    assert len(streams["white_noise"]) >= len(CASES["white_noise"])            # the caller's rule: coded only if strictly smaller
    assert len(streams["run_70000"]) < 300


def test_refusals(shdr):
    import ctypes
    K, lib = shdr._ops, shdr._lib.load()
    with pytest.raises(ValueError, match="deflate_lz_host"):
        K.deflate_lz_host(b"")
    with pytest.raises(ValueError, match="deflate_lz_parse_host"):
        K.deflate_lz_parse_host(b"")
    src = np.frombuffer(CASES["ff_70000"], dtype=np.uint8)
    need = len(K.deflate_lz_host(src.tobytes()))
    out = np.full(need, 0xAB, dtype=np.uint8)
    assert lib.shdr_deflate_lz_host(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.c_void_p(out.ctypes.data), need - 1) == -1
    assert b"too small" in lib.shdr_last_error() and np.all(out == 0xAB)          # nothing written
    assert lib.shdr_deflate_lz_host(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.c_void_p(out.ctypes.data), need) == need


def test_huffman_only_streams_are_unchanged(shdr):
    got = {k: hashlib.sha256(shdr._ops.deflate_huffman_host(CHUNKS[k])).hexdigest() for k in sorted(CHUNKS)}
    assert got == HUFFMAN_ONLY_SHA256


# ---- size: against the Huffman-only encoder, on the bench's content ------------------------------------------------------------------
def stored(encode, chunks):
    """bytes that OpenEXR's rule stores: the stream if it is strictly smaller than the chunk, else the chunk"""
    return sum(min(len(encode(c)), len(c)) for c in chunks)


@pytest.mark.parametrize("kind", ["noisy", "smooth"])
@pytest.mark.parametrize("shape", [(48, 64), (512, 512)], ids=["64x48", "512x512"])
def test_stored_size_against_huffman_only(shdr, shape, kind):
    """HALF, ZIP, the first two chunks.  Measured with this parse (stored / raw, beside zlib level 6):
    64x48 noisy 0.600 (Huffman-only 0.656, zlib 0.559), smooth 0.162 (0.308, 0.061); 512x512 noisy 0.546 (0.625, 0.517), smooth
    0.0228 (0.222, 0.0122): the smooth 512x512 chunks are 0.10 of the Huffman-only size, the bar is one quarter."""
    K = shdr._ops
    chunks = predicted_chunks(bench_content(shape[0], shape[1], 0.02 if kind == "noisy" else 0.0, seed=1 + shape[0]), 16, 2)
    raw = sum(len(c) for c in chunks)
    for c in chunks:
        assert zlib.decompress(K.deflate_lz_host(c)) == c
    lz, huffman, level6 = stored(K.deflate_lz_host, chunks), stored(K.deflate_huffman_host, chunks), stored(lambda c: zlib.compress(c, 6), chunks)
    print("%s %s: stored / raw  device_lz %.4f  Huffman-only %.4f  zlib level 6 %.4f" % (shape, kind, lz / raw, huffman / raw, level6 / raw))
    assert lz < huffman
    if kind == "smooth" and shape == (512, 512):
        assert 4 * lz <= huffman
