"""NumPy restatement of the Radiance adaptive scanline RLE as the device encoder (csrc/hdr_rle.hip) computes it, and the scanline
families the encoder tests share.

The host routine (`rle_component`, csrc/api.cpp) is a greedy loop.  Read as a whole it does this to one component of one line:

  1. stretches   maximal runs of equal bytes;
  2. capped runs every stretch of length L is cut, from its head, into L // 127 runs of 127 and a remainder of L % 127 -- wherever
                 the encoder's cursor was, because every scan for "the next run" starts at a run boundary;
  3. tokens      a capped run of 4 or more is LONG and coded (128 + len, byte).  A GAP is a maximal sequence of short runs between
                 two long runs (or the line's ends).  A gap that is exactly ONE run of 2 or 3 bytes is coded (128 + len, byte); any
                 other gap is coded as literals, in chunks of at most 128 bytes counted from the gap's first byte, each chunk with its
                 length in front.

`encode_component` states exactly that, run by run.  `encode_component_positions` states the same thing the way the kernel does it:
every byte position decides, from two forward scans (its stretch's head, its gap's first byte) and at most six bytes of lookahead,
which bytes it contributes, and an exclusive prefix sum of those contributions is where it writes them -- 64 positions at a time with
the scans carried along, as a wave does.  tests/test_hdr_rle_ref.py holds both byte-equal to the host routine.
"""
import numpy as np

MIN_RUN, MAX_RUN, MAX_LITERAL = 4, 127, 128


def capped_runs(line):
    """[(start, length)] of the capped runs of one component line (steps 1 and 2)"""
    line = np.asarray(line, dtype=np.uint8)
    n = line.size
    heads = np.flatnonzero(np.concatenate(([True], line[1:] != line[:-1])))
    ends = np.concatenate((heads[1:], [n]))
    runs = []
    for s, e in zip(heads.tolist(), ends.tolist()):
        while e - s > MAX_RUN:
            runs.append((s, MAX_RUN))
            s += MAX_RUN
        runs.append((s, e - s))
    return runs


def encode_component(line):
    """bytes of one component of one scanline (step 3)"""
    line = np.asarray(line, dtype=np.uint8)
    out = bytearray()
    gap = []                                        # the short runs since the last long one

    def flush():
        if not gap:
            return
        start, total = gap[0][0], sum(l for _, l in gap)
        if len(gap) == 1 and total >= 2:            # one run of 2 or 3
            out.extend((128 + total, int(line[start])))
        else:
            for c in range(start, start + total, MAX_LITERAL):
                m = min(MAX_LITERAL, start + total - c)
                out.append(m)
                out.extend(line[c:c + m].tobytes())
        gap.clear()

    for s, l in capped_runs(line):
        if l >= MIN_RUN:
            flush()
            out.extend((128 + l, int(line[s])))
        else:
            gap.append((s, l))
    flush()
    return bytes(out)


def encode_component_positions(line, lanes=64):
    """the same bytes from per-position rules, walked as csrc/hdr_rle.hip walks them: `lanes` positions at a time, the two scans and
    the byte count carried from one step to the next (names follow the kernel)"""
    line = np.asarray(line, dtype=np.uint8)
    n = line.size
    d = np.full(n + 1 + lanes + 8, -2, dtype=np.int32)      # d[i + 1] = byte i; -1 before the line, -2 after it
    d[0] = -1
    d[1:n + 1] = line
    out = np.zeros(2 * n + 2, dtype=np.uint8)
    carry_key, carry_gap, carry_short, carry_p = -1, -1, False, 0
    for base in range(0, n, lanes):
        x = np.arange(base, base + lanes)

        def D(k):                                           # byte at x + k for every lane
            return d[base + 1 + k:base + 1 + k + lanes]

        hd = [D(k) != D(k - 1) for k in range(0, 7)]        # hd[k]: position x + k starts a stretch (the end of the line does too)

        def lh(k):                                          # the stretch starting at x + k has 4 or more bytes
            return (D(k) >= 0) & (D(k) == D(k + 1)) & (D(k) == D(k + 2)) & (D(k) == D(k + 3))

        # scan 1: head of the stretch of x, and whether that stretch is long
        key = np.maximum(np.maximum.accumulate(np.where(hd[0], x * 2 + lh(0), -1)), carry_key)
        carry_key = key[-1]
        s0 = key >> 1
        s_k, long_k = s0, (key & 1).astype(bool)
        short = []
        for k in range(0, 4):                               # short[k]: position x + k lies in a short capped run
            if k:
                s_k = np.where(hd[k], x + k, s_k)
                long_k = np.where(hd[k], lh(k), long_k)
            y = x + k
            e = np.where(hd[k + 1], y + 1, np.where(hd[k + 2], y + 2, np.where(hd[k + 3], y + 3, -1)))
            length = e - s_k
            rem = length % MAX_RUN
            short_rest = (e >= 0) & (rem < MIN_RUN) & (y - s_k >= length - rem)
            short.append((D(k) >= 0) & (~long_k | short_rest))
        prev_short = np.concatenate(([carry_short], short[0][:-1]))
        carry_short = short[0][-1]
        # scan 2: first byte of the gap of x
        g = np.maximum(np.maximum.accumulate(np.where(short[0] & ~prev_short, x, -1)), carry_gap)
        carry_gap = g[-1]
        rel = x - g
        # a gap that is one run of 2 or 3: its last byte codes it
        yl = np.where(~short[1], 0, np.where(~short[2], 1, np.where(~short[3], 2, 9)))
        glen = rel + yl + 1
        tok = short[0] & (glen >= 2) & (glen <= 3) & (s0 <= g) & ((yl < 1) | ~hd[1]) & ((yl < 2) | ~hd[2])
        gap_last = ~short[1]
        o = (x - s0) % MAX_RUN
        run_last = (o == MAX_RUN - 1) | hd[1]
        chunk = rel % MAX_LITERAL
        contrib = np.where(D(0) < 0, 0, np.where(~short[0], np.where(run_last, 2, 0),
                                                 np.where(tok, np.where(gap_last, 2, 0), 1 + (chunk == 0))))
        p = carry_p + np.cumsum(contrib) - contrib
        carry_p += int(contrib.sum())
        for i in np.flatnonzero(contrib):
            if not short[0][i]:
                out[p[i]], out[p[i] + 1] = 128 + o[i] + 1, D(0)[i]
            elif tok[i]:
                out[p[i]], out[p[i] + 1] = 128 + glen[i], D(0)[i]
            else:
                out[p[i] + (chunk[i] == 0)] = D(0)[i]
                if gap_last[i] or chunk[i] == MAX_LITERAL - 1:
                    out[p[i] - chunk[i] - (chunk[i] != 0)] = chunk[i] + 1
    return out[:carry_p].tobytes()


def encode_image(rgbe, component=encode_component):
    """scanline bytes of an RGBE image [H, W, 4]: what shdr_rgbe_rle_encode writes"""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    h, w, _ = rgbe.shape
    if w < 8 or w > 32767:
        return rgbe.tobytes()
    out = bytearray()
    for y in range(h):
        out.extend((2, 2, w >> 8, w & 255))
        for c in range(4):
            out.extend(component(rgbe[y, :, c]))
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# scanline families (one component each); every generator returns uint8 [w]
# ---------------------------------------------------------------------------------------------------------------------------------
def _from_runs(w, lengths, first=10):
    """stretches of the given lengths with changing values, cut or filled up to w with single bytes"""
    out = np.empty(w, dtype=np.uint8)
    pos, v = 0, first
    i = 0
    while pos < w:
        l = lengths[i] if i < len(lengths) else 1
        out[pos:pos + l] = v
        pos += l
        v = (v + 37) % 251
        i += 1
    return out


def _literal(rng, n):
    """n bytes without two equal neighbours"""
    return np.cumsum(rng.integers(1, 255, size=n)) % 256


def families(w, rng):
    """name -> line of width w"""
    fam = {}
    fam["constant"] = np.full(w, 77, dtype=np.uint8)
    for r in range(5):                                                      # stretches of 127 k + r
        fam["stretch_127k+%d" % r] = _from_runs(w, [127 + r, 254 + r, 1, 127 + r, r or 2, 381 + r])
    for a in (2, 3, 256):
        fam["alphabet%d" % a] = rng.integers(0, a, size=w).astype(np.uint8)
    for l in (1, 2, 3, 4):
        fam["runs_of_%d" % l] = _from_runs(w, [l] * w)
    for l in (2, 3):
        fam["lone_%d_between_long" % l] = _from_runs(w, [40, l, 50, 7, l, 200, l, 9])
        fam["%d_at_start_and_end" % l] = np.concatenate((_from_runs(w - l, [l, 20, 1, 1, 30] + [5] * w), np.full(l, 3))).astype(np.uint8)
    for n in (127, 128, 129, 256, 257):
        if w >= n + 8:
            lit = _literal(rng, n).astype(np.uint8)
            rest = w - n
            a = np.concatenate((lit, np.full(rest, (int(lit[-1]) + 1) % 256)))                  # gap, then a long run
            b = np.concatenate((np.full(rest, (int(lit[0]) + 1) % 256), lit))                   # long run, then a gap to the end
            fam["gap%d_before_run" % n] = a.astype(np.uint8)
            fam["gap%d_before_end" % n] = b.astype(np.uint8)
    fam["byte_after_long_run"] = np.concatenate((np.full(w - 1, 9), [200])).astype(np.uint8)
    fam["short_rest_after_127"] = _from_runs(w, [128, 5, 129, 1, 130, 2, 2, 254 + 3, 4])
    return fam


def family_image(h, w, seed):
    """uint8 [h, w, 4]: every (row, component) a family line, neighbouring components from different families"""
    rng = np.random.default_rng(seed)
    lines = list(families(w, rng).values())
    img = np.empty((h, w, 4), dtype=np.uint8)
    for y in range(h):
        for c in range(4):
            img[y, :, c] = lines[(seed + 5 * y + 3 * c) % len(lines)]
    return img
