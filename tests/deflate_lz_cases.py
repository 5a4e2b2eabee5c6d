"""Chunks aimed at what can go wrong in the LZ77 deflate encoder (csrc/deflate_lz.h): shared by tests/test_deflate_lz_host.py (zlib
judges the host routine) and tests/test_gpu_deflate_lz.py (the device bytes are the host bytes).

How a chunk makes the chainless parse find a given match: candidate A of a position is the most recent EARLIER-GROUP position with the
same 3-byte hash, one per slot, so whatever lies between two copies of a block must not take the block's slots.  A filler of ONE byte
value does that: it is coded as runs (distance 1) and all of its positions share one slot.  Distances below 64 cannot come from two
copies in one group of 64 positions; a pattern of period d gives them from the second group on."""
import numpy as np

from test_deflate_host import CHUNKS

FILL, STOP = 254, 255                                       # block bytes are drawn below both

DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
DIST_BASE = [1 + sum(1 << e for e in DIST_EXTRA[:c]) for c in range(30)]
LEN_EXTRA = [0] * 8 + [e for e in range(1, 6) for _ in range(4)] + [0]
LEN_BASE = [3 + sum(1 << e for e in LEN_EXTRA[:c]) for c in range(28)] + [258]
assert DIST_BASE[29] == 24577 and DIST_BASE[4] == 5 and LEN_BASE[8] == 11 and LEN_BASE[27] == 227


def distance_code(d):
    return max(c for c in range(30) if DIST_BASE[c] <= d)


def length_code(n):
    """0..28 for the symbols 257..285"""
    return 28 if n == 258 else max(c for c in range(28) if LEN_BASE[c] <= n)


def boundary_distances():
    """every distance that begins or ends a distance code: 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, ... 24577, 32768"""
    return sorted({DIST_BASE[c] for c in range(30)} | {DIST_BASE[c] + (1 << DIST_EXTRA[c]) - 1 for c in range(30)})


def boundary_lengths():
    """every length that begins or ends a length code: 3 .. 10, 11, 12, 13, 14, ... 227, 257, 258"""
    return sorted({LEN_BASE[c] for c in range(29)} | {LEN_BASE[c] + (1 << LEN_EXTRA[c]) - 1 for c in range(28)})


def block(rng, n):
    return rng.integers(0, FILL, n, dtype=np.uint8).tobytes()


def slot(chunk, q):
    """hash3 of csrc/deflate_lz.h for the bytes q, q + 1, q + 2"""
    return (((chunk[q] | chunk[q + 1] << 8 | chunk[q + 2] << 16) * 2654435761) & 0xFFFFFFFF) >> 20


def keeps_its_slot(chunk, p):
    """position 0 is still what the table holds for its slot when the group of position p is looked up"""
    return all(slot(chunk, q) != slot(chunk, 0) for q in range(1, p - p % 64))


def repeat_at(rng, d, n=40):
    """an n-byte block that comes again d bytes later and ends the chunk"""
    if d <= 100:
        return (block(rng, d) * (200 // d + 3))[:128 + d + n]             # period d; the second group finds it
    while True:
        b = block(rng, n)
        chunk = b + bytes([FILL]) * (d - n) + b
        if keeps_its_slot(chunk, d):
            return chunk


def repeat_of(rng, n):
    """an n-byte block, a run, the block again, then a byte that ends the match after exactly n bytes"""
    while True:
        b = block(rng, n)
        chunk = b + bytes([FILL]) * 70 + b + bytes([STOP, 1, 2, 3])
        if keeps_its_slot(chunk, n + 70):
            return chunk


def cases():
    rng = np.random.default_rng(31)
    out = dict(CHUNKS)
    for n in (1, 2, 3, 4, 63, 64, 65, 127, 128, 129):
        out["few_values_%d" % n] = rng.integers(0, 3, n, dtype=np.uint8).tobytes()
    for n in (257, 258, 259, 260, 516, 70000):
        out["run_%d" % n] = b"\x11" * n
    for d in boundary_distances() + [32769]:
        out["distance_%05d" % d] = repeat_at(rng, d)
    for n in boundary_lengths():
        out["length_%03d" % n] = repeat_of(rng, n)
    b = block(rng, 20)
    out["match_ends_the_chunk"] = b + bytes([FILL]) * 100 + b
    out["no_match_at_all"] = bytes(range(255, -1, -1))
    out["one_distance_code"] = b"\x07" * 300
    out["white_noise"] = np.random.default_rng(5).integers(0, 256, 50000, dtype=np.uint8).tobytes()
    return out


CASES = cases()


# ---- the content of tools/exr_write_bench.py, its HALF scanlines and OpenEXR's predictor (as in tests/exr_ref.py) -----------------
def bench_content(h, w, noise, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    base = np.stack((1.0 + xx / w + yy / h, 0.5 + 0.25 * xx / w + 0.1 * yy / h, 2.0 + 3.0 * (xx + yy) / (h + w)), axis=-1)
    if noise:
        base = base * (1.0 + noise * rng.standard_normal(base.shape))
    return base.astype(np.float32)


def predict(raw):
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    t = np.concatenate([a[0::2], a[1::2]])
    d = t.copy()
    d[1:] = t[1:] - t[:-1] + np.uint8(128)
    return d.tobytes()


def predicted_chunks(img, lines, count):
    """the predicted bytes of the first `count` chunks of a HALF file of img [H, W, 3] (channels in the order B, G, R)"""
    half = img.astype(np.float16)
    rows = [b"".join(half[y, :, c].tobytes() for c in (2, 1, 0)) for y in range(img.shape[0])]
    return [predict(b"".join(rows[c * lines:(c + 1) * lines])) for c in range(count)]
