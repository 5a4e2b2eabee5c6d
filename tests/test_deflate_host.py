"""The host routine of the Huffman-only zlib encoder (shdr_deflate_huffman_host, csrc/deflate_huffman.h), through ctypes: zlib's own
inflate is the judge of the streams, and the code lengths are checked through shdr_deflate_huffman_lengths_host."""
import zlib

import numpy as np
import pytest


def fibonacci_chunk():
    """byte counts 1, 1, 2, 3, ... over 24 symbols (121 392 bytes): an unlimited Huffman code can be 24 bits deep"""
    counts, a, b = [], 1, 1
    for _ in range(24):
        counts.append(a)
        a, b = b, a + b
    return b"".join(bytes([7 * s + 3]) * c for s, c in enumerate(counts))


def powers_chunk():
    """byte counts 2, 4, ... 2^18 over 18 symbols (524 286 bytes) beside the end-of-block count of 1: every weight exceeds the sum of
    the smaller ones, so whatever the tie-breaking the unlimited Huffman tree is a chain 18 deep and the 15-bit limit must act"""
    return b"".join(bytes([13 * s + 1]) * (2 << s) for s in range(18))


def chunks():
    rng = np.random.default_rng(11)
    out = {"len%d" % n: rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1, 2, 3, 255, 256, 257)}
    out["one_byte_repeated"] = b"\x2a" * 1000
    out["all_256_values"] = bytes(range(256))
    out["ff_70000"] = b"\xff" * 70000                       # Adler-32 past zlib's 5552-byte window
    out["fibonacci"] = fibonacci_chunk()
    out["powers_of_two"] = powers_chunk()
    out["noisy_ramp"] = (128 + rng.integers(-3, 4, 49152)).astype(np.uint8).tobytes()
    return out


CHUNKS = chunks()


def test_fibonacci_chunk_is_what_it_claims():
    assert len(CHUNKS["fibonacci"]) == 121392 and len(set(CHUNKS["fibonacci"])) == 24


@pytest.mark.parametrize("name", sorted(CHUNKS))
def test_stream_inflates_to_the_chunk(shdr, name):
    chunk = CHUNKS[name]
    stream = shdr._ops.deflate_huffman_host(chunk)
    assert zlib.decompress(stream) == chunk
    d = zlib.decompressobj()
    assert d.decompress(stream) == chunk and d.eof and d.unused_data == b""


@pytest.mark.parametrize("name", sorted(CHUNKS))
def test_code_lengths_are_limited_and_complete(shdr, name):
    chunk = CHUNKS[name]
    lengths = shdr._ops.deflate_huffman_lengths_host(chunk).astype(np.int64)
    used = np.bincount(np.frombuffer(chunk, dtype=np.uint8), minlength=257) > 0
    used[256] = True                                        # end-of-block
    assert lengths.shape == (257,)
    assert np.all(lengths[~used] == 0) and np.all(lengths[used] >= 1) and np.all(lengths[used] <= 15)
    assert int((1 << (15 - lengths[used])).sum()) == 1 << 15          # Kraft sum exactly 1


def bits_of(stream, lo, hi):
    """stream bits lo .. hi - 1 as a list (a byte fills from its bit 0)"""
    return [(stream[i >> 3] >> (i & 7)) & 1 for i in range(lo, hi)]


def value(bits):
    return sum(b << i for i, b in enumerate(bits))


@pytest.mark.parametrize("name", ["len1", "all_256_values", "fibonacci"])
def test_header_fields_and_code_lengths_in_the_stream(shdr, name):
    chunk = CHUNKS[name]
    stream = shdr._ops.deflate_huffman_host(chunk)
    assert stream[:2] == b"\x78\x01"
    f = bits_of(stream, 16, 33)
    assert f[0] == 1                                        # BFINAL
    assert value(f[1:3]) == 2                               # BTYPE: dynamic Huffman
    assert value(f[3:8]) == 0 and value(f[8:13]) == 0       # HLIT = 0 (257 codes), HDIST = 0 (1 code)
    assert value(f[13:17]) == 15                            # HCLEN: all 19
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = bits_of(stream, 33, 33 + 57)
    assert [value(cl[3 * i:3 * i + 3]) for i in range(19)] == [4 if s <= 15 else 0 for s in order]
    body = bits_of(stream, 90, 1122)                        # 258 lengths, each the 4-bit code L, most significant bit first
    got = [int("".join(map(str, body[4 * i:4 * i + 4])), 2) for i in range(258)]
    assert got[:257] == shdr._ops.deflate_huffman_lengths_host(chunk).tolist() and got[257] == 0
    assert stream[-4:] == zlib.adler32(chunk).to_bytes(4, "big")


def unlimited_depth(chunk, deepest):
    """depth of a Huffman tree over the chunk's byte counts and end-of-block, ties resolved towards the deepest or the shallowest tree"""
    import heapq
    hist = np.bincount(np.frombuffer(chunk, dtype=np.uint8))
    heap = [(c, 0) for c in hist[hist > 0].tolist() + [1]]
    heapq.heapify(heap)
    sign = -1 if deepest else 1
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, sign * (max(sign * da, sign * db) + 1)))
    return sign * heap[0][1]


def test_the_length_limit_acts(shdr):
    """Fibonacci counts allow trees up to 24 deep (which one depends on how ties are broken); the powers of two allow only the chain"""
    K = shdr._ops
    assert unlimited_depth(CHUNKS["fibonacci"], deepest=True) > 15
    assert unlimited_depth(CHUNKS["powers_of_two"], deepest=False) == 18
    for name in ("fibonacci", "powers_of_two"):
        lengths = K.deflate_huffman_lengths_host(CHUNKS[name])
        assert lengths.max() <= 15 and int((1 << (15 - lengths[lengths > 0].astype(np.int64))).sum()) == 1 << 15


def test_white_noise_is_reported_as_not_smaller(shdr):
    K = shdr._ops
    noise = np.random.default_rng(5).integers(0, 256, 50000, dtype=np.uint8).tobytes()
    stream = K.deflate_huffman_host(noise)
    assert zlib.decompress(stream) == noise
    assert len(stream) >= len(noise)                        # the caller's rule: coded only if strictly smaller
    ramp = CHUNKS["noisy_ramp"]
    assert len(K.deflate_huffman_host(ramp)) < len(ramp)


def test_refusals(shdr):
    import ctypes
    K, lib = shdr._ops, shdr._lib.load()
    with pytest.raises(ValueError, match="deflate_huffman_host"):
        K.deflate_huffman_host(b"")
    src = np.frombuffer(CHUNKS["ff_70000"], dtype=np.uint8)
    need = len(K.deflate_huffman_host(src.tobytes()))
    out = np.full(need, 0xAB, dtype=np.uint8)
    assert lib.shdr_deflate_huffman_host(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.c_void_p(out.ctypes.data), need - 1) == -1
    assert b"too small" in lib.shdr_last_error() and np.all(out == 0xAB)          # nothing written
    assert lib.shdr_deflate_huffman_host(ctypes.c_void_p(src.ctypes.data), src.size, ctypes.c_void_p(out.ctypes.data), need) == need


@pytest.mark.parametrize("offsets, pad, out_bytes, huffman_ws, lz_ws", [([0, 5, 12, 1012], 8, 1036, 896, 5088), ([0, 1], 0, 1, 320, 384)])
def test_batch_sizes_of_both_encoders(shdr, offsets, pad, out_bytes, huffman_ws, lz_ws):
    """the output bound (the chunks + pad in front of each) and the workspace layouts, C chunks of `total` bytes:
    272 C + 2 align16(8 C) + align16(4 C) Huffman-only, 320 C + the same + align16(4 total) with the parse's tokens"""
    import ctypes
    lib = shdr._lib.load()
    off = np.asarray(offsets, dtype=np.int64)
    for fn, ws in ((lib.shdr_deflate_huffman_batch_sizes, huffman_ws), (lib.shdr_deflate_lz_batch_sizes, lz_ws)):
        out_b, ws_b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert fn(ctypes.c_void_p(off.ctypes.data), off.size - 1, pad, ctypes.byref(out_b), ctypes.byref(ws_b)) == 0
        assert (out_b.value, ws_b.value) == (out_bytes, ws)
