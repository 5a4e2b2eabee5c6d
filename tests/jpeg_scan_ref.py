"""The rules of the JPEG scan preparation (csrc/jpeg_scan.h) restated in NumPy on a bare scan region, and the corpus the host twin and
the kernels are held to.  Independent of the product code: tests/test_jpeg_scan_host.py pins it to jpeg.parse / unstuff / plan.

A region b[0 .. n) is a file from the first byte after its SOS header to its end.  A marker is FF followed by a byte that is not
00, not FF and not D0 .. D7; `end` is the first one.  Before `end`: FF Dn is a restart marker (neither byte kept, a new segment
after it), a 00 after FF is dropped, FF FF sets the fill flag, every other byte is kept."""
import collections

import numpy as np

Scan = collections.namedtuple("Scan", "end end_marker n_rst kept fill bounds stream lengths")
"""end: -1 if none; end_marker: b[end + 1] or -1; bounds: int64 [seg_cap - 1], kept bytes before restart marker k, -1 where there is
no such marker; stream: the kept bytes; lengths: int64 [seg_cap] kept bytes per segment, what follows the last slot in the last"""


def scan(region, seg_cap):
    b = np.frombuffer(bytes(region), dtype=np.uint8).astype(np.int16)
    n = b.size
    nxt = np.concatenate([b[1:], [-1]]) if n else b
    prv = np.concatenate([[-1], b[:-1]]) if n else b
    ff = b == 0xFF
    rst = ff & (nxt >= 0xD0) & (nxt <= 0xD7)
    marker = ff & (nxt > 0) & (nxt != 0xFF) & ~rst
    found = np.flatnonzero(marker)
    end = int(found[0]) if found.size else -1
    stop = end if end >= 0 else n
    inside = np.arange(n) < stop
    rst &= inside
    keep = inside & ~rst & ~((prv == 0xFF) & ((b == 0) | ((b >= 0xD0) & (b <= 0xD7))))
    kept_before = np.cumsum(keep) - keep
    marks = np.flatnonzero(rst)
    bounds = np.full(seg_cap - 1, -1, dtype=np.int64)
    k = min(marks.size, seg_cap - 1)
    bounds[:k] = kept_before[marks[:k]]
    seg_of = np.minimum(np.cumsum(rst)[keep], seg_cap - 1)
    lengths = np.bincount(seg_of, minlength=seg_cap).astype(np.int64)
    return Scan(end, int(b[end + 1]) if end >= 0 else -1, int(marks.size), int(keep.sum()), int(np.any(inside & ff & (nxt == 0xFF))),
                bounds, b[keep].astype(np.uint8), lengths)


def arena(scans):
    """(uint8 arena, int32 dword of every segment) of a batch of Scan: every segment on a dword, pad bytes FF, image after image:
    the placement of jpeg.plan"""
    chunks, dwords_of = [], []
    dword = 0
    for s in scans:
        dwords = (s.lengths + 3) // 4
        first = dword + np.cumsum(dwords) - dwords
        a = np.full(int(dwords.sum()) * 4, 0xFF, dtype=np.uint8)
        seg_of = np.repeat(np.arange(s.lengths.size), s.lengths)
        start = np.cumsum(s.lengths) - s.lengths
        a[(first[seg_of] - dword) * 4 + np.arange(s.kept) - start[seg_of]] = s.stream
        chunks.append(a)
        dwords_of.append(first)
        dword += int(dwords.sum())
    return np.concatenate(chunks), np.concatenate(dwords_of).astype(np.int32)


def _at(length, pos, pattern, fill=0x41):
    """`length` data bytes with `pattern` written at `pos`"""
    b = bytearray([fill]) * length
    b[pos:pos + len(pattern)] = pattern
    return bytes(b)


def crafted(T):
    """[(name, region, seg_cap)]: the cases of the tile size T"""
    H = bytes.fromhex
    out = []
    for m, at in (("T", T), ("2T", 2 * T)):                                # the pair straddles a tile boundary: FF at at - 1
        out.append(("stuffing_across_%s" % m, _at(at + 40, at - 1, H("FF00")) + H("FFD9"), 1))
        out.append(("restart_across_%s" % m, _at(at + 40, at - 1, H("FFD3")) + H("FFD9"), 2))
        out.append(("end_across_%s" % m, _at(at + 40, at - 1, H("FFD9")), 1))
        out.append(("stuffing_then_restart_across_%s" % m, _at(at + 40, at - 3, H("FF00FFD0")) + H("FFD9"), 2))
    out += [
        ("stuffing_first", H("FF00") + b"abc" + H("FFD9"), 1),
        ("restart_first_empty_first_segment", H("FFD0") + b"abc" + H("FFD9"), 2),
        ("two_adjacent_restarts_empty_middle", b"ab" + H("FFD0FFD1") + b"cd" + H("FFD9"), 3),
        ("restart_before_end_empty_last", b"abcde" + H("FFD0FFD9"), 2),
        ("final_lone_ff_no_end", b"abc" + H("FF00") + b"d" + H("FF"), 1),
        ("length_0", b"", 1), ("length_1", b"a", 1), ("length_1_ff", H("FF"), 1), ("length_2", b"ab", 1), ("length_2_end", H("FFD9"), 1),
        ("length_2_stuffing", H("FF00"), 1), ("length_2_restart", H("FFD7"), 2), ("length_2_fill", H("FFFF"), 1),
        ("ignored_after_end", b"abc" + H("FF00") + b"d" + H("FFD9") + b"x" + H("FF00FFD1FFFFFFD8FFE1") + b"yz" + H("FFD9FF"), 1),
        ("fill_before_end", b"ab" + H("FFFF00") + b"c" + H("FFD9"), 1),
        ("fill_then_restart", b"ab" + H("FFFFD2") + b"c" + H("FFD9"), 2),
        ("end_is_sos", b"abc" + H("FFDA000C"), 1), ("end_is_dht", b"abc" + H("FFC4001F"), 1), ("end_is_app1", b"abc" + H("FFE10010"), 1),
        ("zero_after_restart_is_kept", H("FFD000") + b"a" + H("FFD9"), 2),
        ("one_marker_more_than_slots", b"a" + H("FFD0") + b"bb" + H("FFD1") + b"ccc" + H("FFD2") + b"dddd" + H("FFD9"), 3),
        ("many_markers_more_than_slots", b"".join(b"xy" + bytes([0xFF, 0xD0 + k % 8]) for k in range(40)) + H("FFD9"), 4),
        ("markers_and_no_slot_at_all", b"a" + H("FFD0") + b"b" + H("FFD1") + b"c" + H("FFD9"), 1),
        ("one_marker_fewer_than_slots", b"a" + H("FFD0") + b"bb" + H("FFD1") + b"ccc" + H("FFD9"), 4),
        ("no_marker_but_slots", b"abcdefg" + H("FFD9"), 3),
    ]
    return out


ALPHABET = [0x00, 0xFF] + list(range(0xD0, 0xD8)) + [0xD9, 0x41, 0x7E, 0x01]
WEIGHTS = np.array([6, 5] + [1] * 8 + [0.15, 6, 6, 6], dtype=np.float64)


def random_cases(T, count=320, seed=20):
    """seeded strings over a small weighted alphabet, lengths around 1, T, 2T and 3T +- 2; seg_cap from 1 to a few more than they hold"""
    rng = np.random.default_rng(seed)
    out = []
    centres = [1, T, 2 * T, 3 * T]
    for i in range(count):
        n = max(0, centres[i % 4] + int(rng.integers(-2, 3)) + (int(rng.integers(0, 40)) if i % 8 >= 4 else 0))
        w = WEIGHTS.copy()
        if i % 3:
            w[10] = 0.0                                                    # no EOI in two of three: the end comes from FF + data, or never
        if i % 5 == 0:
            w[11:] *= 40                                                   # mostly data: the end lies deep in the string
        b = rng.choice(ALPHABET, size=n, p=w / w.sum()).astype(np.uint8)
        if i % 2 == 0 and n > 2:                                           # no marker before a random cut: the end lies anywhere, or nowhere
            cut = int(rng.integers(0, n + 1))
            p = np.flatnonzero((b[:-1] == 0xFF) & np.isin(b[1:], [0xD9, 0x41, 0x7E, 0x01]))
            p = p[p < cut]
            b[p + 1] = np.where(rng.random(p.size) < 0.5, 0x00, 0xD0 + (p & 7)).astype(np.uint8)
        out.append(("random_%03d_n%d" % (i, n), b.tobytes(), int(rng.integers(1, 9))))
    return out


def long_case(T, chunk_tiles):
    """one region of more than T * chunk_tiles bytes -- more than one workgroup of the cross-tile prefix sum, whose workgroups take
    chunk_tiles tiles each -- with stuffing and restart markers all along and its end in the last tile"""
    rng = np.random.default_rng(21)
    n = T * (chunk_tiles + 44) + 5
    b = rng.integers(0, 0xFF, n, dtype=np.uint8)                           # no FF
    pos = np.sort(rng.choice(np.arange(0, n - 64, 2), size=n // 37, replace=False))       # even positions: the pairs do not overlap
    kinds = rng.integers(0, 3, pos.size)
    b[pos] = 0xFF
    b[pos + 1] = np.where(kinds == 0, 0x00, np.where(kinds == 1, 0xD0 + (np.arange(pos.size) & 7), b[pos + 1] & 0x7F)).astype(np.uint8)
    b[pos[kinds == 2]] = 0x55                                              # (a third of the sites stay plain data)
    b[n - 40], b[n - 39] = 0xFF, 0xD9
    return ("long_%d_bytes" % n, b.tobytes(), int((kinds == 1).sum()) + 1)


def corpus(T, chunk_tiles):
    return crafted(T) + random_cases(T) + [long_case(T, chunk_tiles)]


if __name__ == "__main__":                                                # the corpus as files, for tools/jpeg_scan_sweep.cpp
    import argparse
    import os
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True, help="directory that receives <name>.<seg_cap>.scan")
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--chunk-tiles", type=int, default=256)
    args = ap.parse_args()
    os.makedirs(args.dump, exist_ok=True)
    for name, region, cap in corpus(args.tile, args.chunk_tiles):
        with open(os.path.join(args.dump, "%s.%d.scan" % (name, cap)), "wb") as f:
            f.write(region)
