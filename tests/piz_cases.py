"""The PIZ chunks that the CPU tests (host twin against piz_ref) and the GPU tests (kernels against the host twin) share, built once
per process with piz_ref's encoder.

    python tests/piz_cases.py --dump DIR     writes every case as DIR/<name>.<width>.<rows>.<words>.piz for tools/piz_sweep.cpp
                                             (<words>: one digit per channel)

A Case is (name, chunk bytes, width, rows, chan_words, raw): raw is the scanline bytes the chunk must decode to, or None for chunks
assembled at the level of the Huffman stream (their reference is piz_ref.decode_chunk alone)."""
import collections
import functools
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import piz_ref  # noqa: E402

Case = collections.namedtuple("Case", "name data width rows words raw")

WIDTHS = (1, 2, 9, 31, 32, 33, 65, 100)
ROWS = (1, 5, 17, 32)
CHANNELS = {"half": (1, 1, 1), "float": (2, 2, 2), "mixed": (1, 1, 1, 1, 2)}        # mixed: A, B, G, R HALF and Z FLOAT
CONTENTS = ("constant", "ramp", "noise14", "noise16", "runs")


def content(kind, rng, rows, n):
    """uint16 [rows, n]: one kind of sample words for a chunk's scanlines"""
    if kind == "constant":
        return np.full((rows, n), 0x3C00, dtype=np.uint16)
    if kind == "ramp":
        return ((np.arange(rows)[:, None] * 7 + np.arange(n)[None, :]) * 3 & 0x3FFF).astype(np.uint16)
    if kind == "noise14":
        return rng.integers(0, 1 << 14, (rows, n)).astype(np.uint16)
    if kind == "noise16":
        return rng.integers(0, 1 << 16, (rows, n)).astype(np.uint16)
    out = np.zeros((rows, n), dtype=np.uint16)                         # runs: long stretches of equal values, a few others
    out[:, n // 2:] = 0x4000
    out[rng.integers(0, rows), rng.integers(0, n)] = 0x1234
    return out


def image_case(name, kind, width, rows, words, seed, **enc):
    rng = np.random.default_rng(seed)
    raw = content(kind, rng, rows, width * sum(words)).astype("<u2").tobytes()
    enc.setdefault("force16", kind == "noise16")
    return Case(name, piz_ref.encode_chunk(raw, width, rows, words, **enc), width, rows, tuple(words), raw)


def assemble(block, present, lo=None, hi=None):
    """a chunk from a ready Huffman block; present: the values of the bitmap"""
    bits = np.zeros(65536, dtype=bool)
    bits[list(present)] = True
    bitmap = np.packbits(bits, bitorder="little")
    bitmap[0] &= 0xFE
    nz = np.flatnonzero(bitmap)
    if lo is None:
        lo, hi = (int(nz[0]), int(nz[-1])) if nz.size else (8191, 0)
    return struct.pack("<HH", lo, hi) + (bitmap[lo:hi + 1].tobytes() if lo <= hi else b"") + struct.pack("<i", len(block)) + block


def ladder_lengths(top):
    """a complete code of top + 1 symbols 0 .. top: lengths 1, 2, ..., top, top (top up to 58: far beyond the first-level table)"""
    return {s: min(s + 1, top) for s in range(top + 1)}


def stream_cases():
    out = []
    # fixed 8-bit codes: tokens of 8 (a value) and 16 (a run) bits at known bit positions.  With 128-bit subsequences a run is the
    # first token of subsequence 1, runs cross the borders of several subsequences, and a run token itself straddles a border
    flat = {s: 8 for s in range(0, 200)}                               # symbols 0 .. 198 and the run code 199
    toks = [(s, None) for s in range(1, 17)] + [("run", 200), (7, None)] * 3 + [(s % 150, None) for s in range(15)] + [("run", 255)] * 9
    n = sum(k if s == "run" else 1 for s, k in toks)
    toks += [(3, None)] * (100 * 32 - n)
    out.append(Case("run_first_in_subsequence", assemble(piz_ref.huf_encode(tokens=toks, lengths=flat, im=0, iM=199), range(0, 400)),
                    100, 32, (1,), None))
    # long codes: a ladder up to 58 bits, skewed use, every symbol at least once; both table forms of zero runs around it
    for top, long_runs in ((20, True), (58, False), (58, True)):
        lengths = {10 + s: l for s, l in ladder_lengths(top).items()}  # symbols 10 .. 10 + top, the last one the run code
        lengths[700] = lengths.pop(10 + top)                           # ... moved far away: a long zero run in the table
        rng = np.random.default_rng(top)
        vals = [10 + int(v) for v in np.minimum(rng.geometric(0.5, 31 * 17) - 1, top - 1)]
        vals[5:5 + top] = range(10, 10 + top)
        toks = piz_ref.tokens_of(vals, runs=True)
        out.append(Case("ladder%d_%s" % (top, "long" if long_runs else "short"),
                        assemble(piz_ref.huf_encode(tokens=toks, lengths=lengths, im=3, iM=700, long_runs=long_runs), range(0, 20000)),
                        31, 17, (1,), None))
    # an incomplete code in which a short code is a prefix of a longer one (lengths 1 and 3 alone): the shortest wins
    toks = [(5, None)] * 9
    out.append(Case("incomplete_prefix", assemble(piz_ref.huf_encode(tokens=toks, lengths={5: 1, 9: 3}, im=5, iM=9), range(0, 64)),
                    9, 1, (1,), None))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out, k = [], 0
    for width in WIDTHS:                                               # every shape once, contents and channel sets in turn
        for rows in ROWS:
            kind, chans = CONTENTS[k % len(CONTENTS)], list(CHANNELS)[k % len(CHANNELS)]
            out.append(image_case("%s_%s_%dx%d" % (kind, chans, width, rows), kind, width, rows, CHANNELS[chans], 100 + k))
            k += 1
    for width, rows in ((33, 17), (100, 32)):                          # every content with every channel set at two awkward shapes
        for kind in CONTENTS:
            for chans, words in CHANNELS.items():
                out.append(image_case("%s_%s_%dx%d_b" % (kind, chans, width, rows), kind, width, rows, words, 500 + len(out)))
    out.append(image_case("noise14_noruns_65x17", "noise14", 65, 17, (1, 1, 1), 7, runs=False))
    out.append(image_case("runs_shorttable_65x32", "runs", 65, 32, (1, 2), 8, long_runs=False))
    out.append(image_case("ramp_forced16_33x5", "ramp", 33, 5, (1, 1, 1), 9, force16=True))
    return tuple(out + stream_cases())


@functools.lru_cache(maxsize=None)
def small_cases():
    """two chunks small enough for every single-bit flip and every truncation"""
    raw = np.random.default_rng(1).integers(0, 48, 3 * 2 * 3).astype("<u2").tobytes()   # small values: a bitmap of 6 bytes
    a = Case("small_noise", piz_ref.encode_chunk(raw, 3, 2, (1, 2)), 3, 2, (1, 2), raw)
    toks = [(4, None), ("run", 3), (9, None), (4, None), ("run", 2), (6, None)]
    b = Case("small_runs", assemble(piz_ref.huf_encode(tokens=toks), (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 300)), 3, 3, (1,), None)
    return a, b


def mutations(data):
    """every truncation and every single-bit flip of a chunk"""
    for cut in range(len(data)):
        yield "cut%d" % cut, data[:cut]
    for bit in range(8 * len(data)):
        m = bytearray(data)
        m[bit >> 3] ^= 1 << (bit & 7)
        yield "flip%d" % bit, bytes(m)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--dump":
        sys.exit(__doc__)
    os.makedirs(sys.argv[2], exist_ok=True)
    for c in cases() + small_cases():
        with open(os.path.join(sys.argv[2], "%s.%d.%d.%s.piz" % (c.name, c.width, c.rows, "".join(map(str, c.words)))), "wb") as f:
            f.write(c.data)
    print(len(cases()) + 2, "chunks written to", sys.argv[2])
