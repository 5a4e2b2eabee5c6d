"""The chunks that the PIZ encoder's CPU tests (host twin against piz_ref) and GPU tests (kernels against the host twin) share, built once
per process.  A Chunk is (name, raw scanline bytes, width, rows, chan_words).

Two chunks are built backwards, from the wavelet coefficients they must have: the coefficients are decoded with piz_ref's inverse
wavelet into pixel ranks, and the ranks are the pixels.  Each checks itself with piz_ref's forward transform before it is handed out."""
import collections
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import piz_cases  # noqa: E402
import piz_ref  # noqa: E402

Chunk = collections.namedtuple("Chunk", "name raw width rows words")

STRETCH_REPEATS = (2, 3, 255, 256, 258, 510, 511)
TABLE_ZEROS = (1, 5, 6, 261, 262, 267)


def value_sequence(raw, width, rows, words):
    """the chunk's value sequence as piz_ref.encode_chunk builds it: LUT, forward wavelet, channels concatenated"""
    planes = piz_ref._planes_of(raw, width, rows, words)
    present = np.zeros(65536, dtype=bool)
    for p in planes:
        present[p.reshape(-1)] = True
    present[0] = True
    forward = np.cumsum(present) - 1
    mx = int(present.sum()) - 1
    values = []
    for p in planes:
        q = forward[p]
        for j in range(q.shape[2]):
            q[:, :, j] = piz_ref.wav_encode(q[:, :, j], mx)
        values.append(q.reshape(-1))
    return np.concatenate(values)


def stretches(seq):
    """[(start, value, length)] of the maximal stretches of equal values"""
    seq = np.asarray(seq)
    starts = np.concatenate([[0], np.flatnonzero(np.diff(seq)) + 1])
    lens = np.diff(np.concatenate([starts, [seq.size]]))
    return list(zip(starts.tolist(), seq[starts].tolist(), lens.tolist()))


def stretch_chunk():
    """65 x 32, three HALF channels: zero stretches of exactly STRETCH_REPEATS repeats among the coefficients of channel 0, and one
    stretch that runs from the end of channel 0 into channel 1.  Everything else alternates between 1 and 2."""
    width, rows, words = 65, 32, (1, 1, 1)
    n = width * rows
    base = 8                                                           # the coarsest coefficients: keeps every pixel rank >= 0
    coef = np.empty(3 * n, dtype=np.int64)
    coef[0::2], coef[1::2] = 1, 2
    coarse = [k * n + x for k in range(3) for x in (0, 32)]            # (y, x) = (0, 0) and (0, 32): the low-pass pair of the last level
    at = 33                                                            # behind them in channel 0
    for rep in sorted(STRETCH_REPEATS, reverse=True):
        coef[at - 1], coef[at + rep + 1] = 1, 2
        coef[at:at + rep + 1] = 0
        at += rep + 3
    assert at < n - 70
    for c in coarse:
        coef[c] = base
    coef[n - 2:2 * n] = 0                                              # the last two of channel 0 and all of channel 1
    q = np.stack([piz_ref.wav_decode(coef[k * n:(k + 1) * n].reshape(rows, width), 1000) for k in range(3)])   # the 14-bit pair
    assert q.max() < 0x8000, "a pixel rank below 0"
    raw = np.ascontiguousarray(q.transpose(1, 0, 2)).astype("<u2").tobytes()      # scanlines: row, channel, x
    found = stretches(value_sequence(raw, width, rows, words))
    reps = [l - 1 for _, _, l in found]
    for rep in STRETCH_REPEATS:
        assert rep in reps, "no stretch of %d repeats" % rep
    assert any(s < n and s + l >= 2 * n for s, _, l in found), "no stretch crosses a channel border"
    return Chunk("stretches_65x32", raw, width, rows, words)


def table_chunk():
    """one HALF channel, 2 rows (one wavelet level: every 2 x 2 block on its own): the used symbols are 0 .. 599 and six more, with
    TABLE_ZEROS unused symbols between them.  A block (r, r, r, r) uses symbol r; a block (b, a, b, a) with b - a even uses the
    symbols (a + b) / 2 and b - a only: that is how the ranks of a gap are pixels and yet no symbols."""
    dense = 600
    quads = [(r, r) for r in range(dense)]
    s = dense - 1                                                      # the used symbol below the next gap
    for g in TABLE_ZEROS:
        t = s + g + 1
        quads.append((t, t))
        quads += [(2 * t - a, a) for a in range(s + 1, t)]
        s = t
    width = 2 * len(quads)
    img = np.empty((2, width), dtype=np.int64)
    for k, (b, a) in enumerate(quads):
        img[:, 2 * k], img[:, 2 * k + 1] = b, a
    assert np.array_equal(np.unique(img), np.arange(img.max() + 1)), "every rank must be a pixel"
    raw = img.astype("<u2").tobytes()
    seq = value_sequence(raw, width, 2, (1,))
    used = np.zeros(int(seq.max()) + 2, dtype=bool)
    used[seq] = True
    used[-1] = True                                                    # the run code
    zeros = [l for _, v, l in stretches(used[int(seq.min()):]) if not v]
    assert sorted(zeros) == sorted(TABLE_ZEROS), zeros
    return Chunk("table_zeros_%dx2" % width, raw, width, 2, (1,))


@functools.lru_cache(maxsize=None)
def chunks():
    out = [Chunk(c.name, c.raw, c.width, c.rows, tuple(c.words)) for c in piz_cases.cases() if c.raw is not None]
    out.append(Chunk("zeros_9x5", bytes(2 * 9 * 5 * 3), 9, 5, (1, 1, 1)))
    out.append(Chunk("constant_33x17", np.full(33 * 17 * 3, 0x3C00, dtype="<u2").tobytes(), 33, 17, (1, 2)))
    ordered = np.arange(100 * 32 * 6, dtype="<u2")
    out.append(Chunk("ordered_100x32", ordered.tobytes(), 100, 32, (2, 2, 2)))
    out.append(Chunk("shuffled_100x32", np.random.default_rng(5).permutation(ordered).astype("<u2").tobytes(), 100, 32, (2, 2, 2)))
    out.append(stretch_chunk())
    out.append(table_chunk())
    out.append(Chunk("one_pixel", np.array([0x3C00, 0x3800, 0x3400], dtype="<u2").tobytes(), 1, 1, (1, 1, 1)))
    return tuple(out)
