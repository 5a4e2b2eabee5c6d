"""An independent PIZ encoder and decoder for the tests, in Python / NumPy, written from the format's rules (restated from memory of
OpenEXR 2.x; not pinned against libOpenEXR, which is not available here) and not from the product's csrc/piz.h.

Chunk (little-endian): u16 minNonZero, u16 maxNonZero, bitmap[min .. max] (if min <= max) of an 8192-byte bitmap of the 16-bit values
present, i32 length, `length` bytes of Huffman block = u32 im, iM, tableLength, nBits, reserved; the 6-bit code-length table of symbols
im .. iM (63: 8 more bits + 6 zeros; 59 .. 62: 2 .. 5 zeros); from the next byte nBits bits of code words, most significant bit first.
Symbol iM is the run code: 8 bits of count follow and the previous value is repeated.  The values are the wavelet coefficients of the
channels' word planes; after the inverse wavelet they go through the reverse LUT.

The encoder can be told to force paths: force16 (a full bitmap, hence the 16-bit wavelet pair), runs on or off, a given set of code
lengths, only the short zero-run form of the table.  Where an incomplete length set makes a short code a prefix of a longer one, the
decoder takes the shortest length whose code range holds the bits."""
import heapq
import struct

import numpy as np

import exr_ref

PIZ = 4
LINES = 32
MAX_LEN = 58
WORDS = {exr_ref.UINT: 2, exr_ref.HALF: 1, exr_ref.FLOAT: 2}


class PizError(ValueError):
    pass


# ---- the wavelet pairs ------------------------------------------------------------------------------------------------------
def _s16(x):
    x = np.asarray(x, dtype=np.int64) & 0xFFFF
    return np.where(x >= 0x8000, x - 0x10000, x)


def dec14(l, h):
    ls, hs = _s16(l), _s16(h)
    a = _s16(ls + (hs & 1) + (hs >> 1))
    b = _s16(a - hs)
    return a & 0xFFFF, b & 0xFFFF


def dec16(l, h):
    l, h = np.asarray(l, dtype=np.int64) & 0xFFFF, np.asarray(h, dtype=np.int64) & 0xFFFF
    b = (l - (h >> 1)) & 0xFFFF
    a = (h + b - 0x8000) & 0xFFFF
    return a, b


def enc14(a, b):
    """the inverse of dec14 (a bijection of 16-bit pairs)"""
    h = _s16(_s16(a) - _s16(b))
    l = _s16(_s16(a) - (h & 1) - (h >> 1))
    return l & 0xFFFF, h & 0xFFFF


def enc16(a, b):
    a, b = np.asarray(a, dtype=np.int64) & 0xFFFF, np.asarray(b, dtype=np.int64) & 0xFFFF
    h = (a - b + 0x8000) & 0xFFFF
    l = (b + (h >> 1)) & 0xFFFF
    return l, h


def _levels(nx, ny):
    n = min(nx, ny)
    p = 1
    while 2 * p <= n:
        p *= 2
    out = []
    p2, p = p, p >> 1
    while p >= 1:
        out.append((p, p2))
        p2, p = p, p >> 1
    return out


def wav_decode_loops(plane, mx, levels=None):
    """the level schedule as the format states it, element by element; plane: int array [ny, nx] (a copy is returned)"""
    a = np.array(plane, dtype=np.int64)
    ny, nx = a.shape
    dec = dec14 if mx < 16384 else dec16

    def d(l, h):
        x, y = dec(l, h)
        return int(x), int(y)
    for p, p2 in (_levels(nx, ny) if levels is None else levels):
        y = 0
        while y <= ny - p2:
            x = 0
            while x <= nx - p2:
                i00, i10 = d(a[y, x], a[y + p, x])
                i01, i11 = d(a[y, x + p], a[y + p, x + p])
                a[y, x], a[y, x + p] = d(i00, i01)
                a[y + p, x], a[y + p, x + p] = d(i10, i11)
                x += p2
            if nx & p:
                a[y, x], a[y + p, x] = d(a[y, x], a[y + p, x])
            y += p2
        if ny & p:
            x = 0
            while x <= nx - p2:
                a[y, x], a[y, x + p] = d(a[y, x], a[y, x + p])
                x += p2
    return a


def _wav(plane, mx, forward, levels=None):
    a = np.array(plane, dtype=np.int64)
    ny, nx = a.shape
    if mx < 16384:
        fn = enc14 if forward else dec14
    else:
        fn = enc16 if forward else dec16
    lv = _levels(nx, ny) if levels is None else levels
    for p, p2 in (reversed(lv) if forward else lv):
        by, bx = (ny - p2) // p2 + 1 if ny >= p2 else 0, (nx - p2) // p2 + 1 if nx >= p2 else 0
        ys, xs = by * p2, bx * p2
        A, B = a[0:ys:p2, 0:xs:p2], a[0:ys:p2, p:xs:p2]
        C, D = a[p:ys:p2, 0:xs:p2], a[p:ys:p2, p:xs:p2]
        if forward:
            i00, i01 = fn(A, B)
            i10, i11 = fn(C, D)
            nA, nC = fn(i00, i10)
            nB, nD = fn(i01, i11)
        else:
            i00, i10 = fn(A, C)
            i01, i11 = fn(B, D)
            nA, nB = fn(i00, i01)
            nC, nD = fn(i10, i11)
        a[0:ys:p2, 0:xs:p2], a[0:ys:p2, p:xs:p2], a[p:ys:p2, 0:xs:p2], a[p:ys:p2, p:xs:p2] = nA, nB, nC, nD
        if nx & p:
            a[0:ys:p2, xs], a[p:ys:p2, xs] = fn(a[0:ys:p2, xs], a[p:ys:p2, xs])
        if ny & p:
            a[ys, 0:xs:p2], a[ys, p:xs:p2] = fn(a[ys, 0:xs:p2], a[ys, p:xs:p2])
    return a


def wav_decode(plane, mx):
    return _wav(plane, mx, False)


def wav_encode(plane, mx):
    return _wav(plane, mx, True)


def wav_decode_strips(plane, mx):
    """the strip form: aligned strips of P columns (P the largest power of two <= min(nx, ny)), each decoded on its own with the
    whole plane's level schedule"""
    a = np.array(plane, dtype=np.int64)
    ny, nx = a.shape
    lv = _levels(nx, ny)
    P = lv[0][1] if lv else 1
    for x0 in range(0, nx, P):
        a[:, x0:x0 + P] = _wav(a[:, x0:x0 + P], mx, False, levels=lv)
    return a


# ---- Huffman --------------------------------------------------------------------------------------------------------------------
def canonical_codes(lengths):
    """lengths: {symbol: length 1 .. 58} -> {symbol: code}; ValueError when over-subscribed"""
    n = [0] * (MAX_LEN + 1)
    for l in lengths.values():
        if not 1 <= l <= MAX_LEN:
            raise ValueError("code length %r" % (l,))
        n[l] += 1
    if sum(n[l] << (MAX_LEN - l) for l in range(1, MAX_LEN + 1)) > 1 << MAX_LEN:
        raise PizError("over-subscribed code lengths")
    c = 0
    for l in range(MAX_LEN, 0, -1):
        nc = (c + n[l]) >> 1
        n[l] = c
        c = nc
    codes = {}
    for s in sorted(lengths):
        codes[s] = n[lengths[s]]
        n[lengths[s]] += 1
    return codes


def huffman_lengths(freq):
    """{symbol: count > 0} -> {symbol: length}, an optimal complete code (one symbol alone gets length 1)"""
    if len(freq) == 1:
        return {next(iter(freq)): 1}
    heap = [(f, s, None, None) for s, f in sorted(freq.items())]
    heapq.heapify(heap)
    tick = 1 << 20
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, a, b))
        tick += 1
    out = {}
    stack = [(heap[0], 0)]
    while stack:
        (f, s, a, b), d = stack.pop()
        if a is None:
            out[s] = d
        else:
            stack.append((a, d + 1))
            stack.append((b, d + 1))
    if max(out.values()) > MAX_LEN:
        raise ValueError("code longer than 58 bits")
    return out


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v = (self.v << bits) | (int(value) & ((1 << bits) - 1))
        self.n += bits

    def bytes(self):
        pad = -self.n % 8
        return ((self.v << pad).to_bytes((self.n + pad) // 8, "big")) if self.n else b""


def tokens_of(values, runs=True, min_run=3):
    """[(symbol, None) | ("run", count)] for a sequence of 16-bit values"""
    v = [int(x) for x in values]
    out, i = [], 0
    while i < len(v):
        out.append((v[i], None))
        j = i + 1
        while j < len(v) and v[j] == v[i]:
            j += 1
        rep = j - i - 1
        if runs and rep >= min_run:
            while rep > 0:
                k = min(rep, 255)
                out.append(("run", k))
                rep -= k
        else:
            out.extend([(v[i], None)] * rep)
        i = j
    return out


def pack_table(lengths, im, iM, long_runs=True):
    """the 6-bit code-length table of symbols im .. iM; long_runs False: only the 2 .. 5 form (59 .. 62) of zero runs"""
    bits = _Bits()
    s = im
    while s <= iM:
        l = lengths.get(s, 0)
        if l:
            bits.put(l, 6)
            s += 1
            continue
        z = 1
        while z < 255 + 6 and s + z <= iM and not lengths.get(s + z, 0):
            z += 1
        if long_runs and z >= 6:
            z = min(z, 255 + 6)
            bits.put(63, 6)
            bits.put(z - 6, 8)
        elif z >= 2:
            z = min(z, 5)
            bits.put(59 + z - 2, 6)
        else:
            bits.put(0, 6)
        s += z
    return bits.bytes()


def huf_encode(values=None, runs=True, lengths=None, long_runs=True, tokens=None, im=None, iM=None, n_bits=None, min_run=3):
    """values (or ready tokens) -> the Huffman block.  lengths: a forced {symbol: length} (the run code is symbol iM); default: an
    optimal code of the tokens' frequencies, in which the run code always has a place.  n_bits: a forced nBits field."""
    toks = tokens_of(values, runs, min_run) if tokens is None else list(tokens)
    syms = [t[0] for t in toks if t[0] != "run"]
    if iM is None:
        iM = (max(syms) if syms else 0) + 1
        if lengths:
            iM = max(iM, max(lengths))
    if im is None:
        im = min(syms) if syms else 0
        if lengths:
            im = min(im, min(lengths))
    if lengths is None:
        freq = {iM: 1}
        for t in toks:
            k = iM if t[0] == "run" else t[0]
            freq[k] = freq.get(k, 0) + 1
        lengths = huffman_lengths(freq)
    codes = canonical_codes(lengths)
    data = _Bits()
    for s, k in toks:
        if s == "run":
            data.put(codes[iM], lengths[iM])
            data.put(k, 8)
        else:
            data.put(codes[s], lengths[s])
    table = pack_table(lengths, im, iM, long_runs)
    return struct.pack("<IIIII", im, iM, len(table), data.n if n_bits is None else n_bits, 0) + table + data.bytes()


def huf_encode_fast(values, min_run=3):
    """huf_encode(values) with its defaults, byte for byte, in NumPy (for files too large for the token loop)"""
    v = np.asarray(values, dtype=np.int64).reshape(-1)
    starts = np.concatenate([[0], np.flatnonzero(np.diff(v)) + 1])
    lens = np.diff(np.concatenate([starts, [v.size]]))
    rep = lens - 1
    use_run = rep >= min_run
    nrun = np.where(use_run, -(-rep // 255), 0)
    ntok = np.where(use_run, 1 + nrun, lens)
    first = np.concatenate([[0], np.cumsum(ntok)])
    sym = np.repeat(v[starts], ntok)
    k = np.arange(first[-1]) - np.repeat(first[:-1], ntok)             # the token's index within its stretch of equal values
    is_run = np.repeat(use_run, ntok) & (k >= 1)
    rep_t, nrun_t = np.repeat(rep, ntok), np.repeat(nrun, ntok)
    count = np.where(k == nrun_t, rep_t - 255 * (nrun_t - 1), 255)
    iM, im = int(sym.max()) + 1, int(sym.min())
    used, n_used = np.unique(sym[~is_run], return_counts=True)
    freq = dict(zip(used.tolist(), n_used.tolist()))
    freq[iM] = 1 + int(is_run.sum())
    lengths = huffman_lengths(freq)
    codes = canonical_codes(lengths)
    code_of, len_of = np.zeros(iM + 1, dtype=np.int64), np.zeros(iM + 1, dtype=np.int64)
    for s, l in lengths.items():
        code_of[s], len_of[s] = codes[s], l
    which = np.where(is_run, iM, sym)
    code, ln = code_of[which], len_of[which]
    pos = np.concatenate([[0], np.cumsum(ln + 8 * is_run)])
    n_bits = int(pos[-1])
    pos = pos[:-1]
    bits = np.zeros(n_bits, dtype=np.uint8)
    for j in range(int(ln.max())):
        sel = ln > j
        bits[pos[sel] + j] = (code[sel] >> (ln[sel] - 1 - j)) & 1
    at, cnt = pos[is_run] + ln[is_run], count[is_run]
    for j in range(8):
        bits[at + j] = (cnt >> (7 - j)) & 1
    table = pack_table(lengths, im, iM)
    return struct.pack("<IIIII", im, iM, len(table), n_bits, 0) + table + np.packbits(bits).tobytes()


def huf_decode(block, n_values):
    """the Huffman block -> n_values 16-bit values (list); PizError on anything wrong"""
    if len(block) < 20:
        raise PizError("short Huffman block")
    im, iM, _, n_bits, _ = struct.unpack_from("<IIIII", block, 0)
    if im >= 65537 or iM >= 65537 or im > iM:
        raise PizError("im / iM")
    body = block[20:]
    total = 8 * len(body)
    stream = int.from_bytes(body, "big") if body else 0

    def take(pos, k):                         # k bits from bit pos, zero beyond the end
        if pos + k <= total:
            return (stream >> (total - pos - k)) & ((1 << k) - 1)
        return ((stream << (pos + k - total)) >> 0) & ((1 << k) - 1)
    lengths, s, pos = {}, im, 0
    while s <= iM:
        if pos + 6 > total:
            raise PizError("table truncated")
        l = take(pos, 6)
        pos += 6
        if l == 63:
            if pos + 8 > total:
                raise PizError("table truncated")
            z = take(pos, 8) + 6
            pos += 8
        elif l >= 59:
            z = l - 59 + 2
        else:
            if l:
                lengths[s] = l
            s += 1
            continue
        if s + z > iM + 1:
            raise PizError("zero run past iM + 1")
        s += z
    codes = canonical_codes(lengths)
    by_len = {}
    for sym, l in lengths.items():
        by_len.setdefault(l, {})[codes[sym]] = sym
    order = sorted(by_len)
    data_at = (pos + 7) // 8 * 8
    if n_bits == 0:
        raise PizError("no data")
    if n_bits > total - data_at:
        raise PizError("nBits beyond the data")
    end = data_at + n_bits
    out, pos, prev = [], data_at, None
    while pos < end:
        sym = None
        for l in order:
            sym = by_len[l].get(take(pos, l))
            if sym is not None:
                break
        if sym is None:
            raise PizError("bad code")
        if pos + l > end:
            raise PizError("data truncated")
        pos += l
        if sym == iM:
            if pos + 8 > end:
                raise PizError("data truncated")
            k = take(pos, 8)
            pos += 8
            if prev is None:
                raise PizError("run with no previous value")
            if len(out) + k > n_values:
                raise PizError("too many values")
            out.extend([prev] * k)
        else:
            if len(out) + 1 > n_values:
                raise PizError("too many values")
            out.append(sym)
            prev = sym
    if len(out) != n_values:
        raise PizError("too few values")
    return out


# ---- chunks -----------------------------------------------------------------------------------------------------------------
def _planes_of(raw, width, rows, chan_words):
    """scanline bytes -> [uint16 array [rows, width, words]] per channel"""
    row = np.frombuffer(bytes(raw), dtype="<u2").reshape(rows, -1)
    out, at = [], 0
    for w in chan_words:
        out.append(row[:, at:at + width * w].reshape(rows, width, w).astype(np.int64))
        at += width * w
    return out


def encode_chunk(raw, width, rows, chan_words, force16=False, fast=False, **huf):
    """the scanline bytes of a chunk (rows x channels x width samples, little-endian) -> its PIZ bytes.  huf: huf_encode's options;
    huf["lengths"] may be a function of the tokens' symbol list that returns the forced lengths; fast: huf_encode_fast."""
    planes = _planes_of(raw, width, rows, chan_words)
    present = np.zeros(65536, dtype=bool)
    for p in planes:
        present[p.reshape(-1)] = True
    if force16:
        present[:] = True
    bitmap = np.packbits(present, bitorder="little")
    stored = bitmap.copy()
    stored[0] &= 0xFE                                                  # value 0 is implied
    nz = np.flatnonzero(stored)
    lo, hi = (int(nz[0]), int(nz[-1])) if nz.size else (8191, 0)
    present[0] = True
    forward = np.cumsum(present) - 1                                   # value -> index
    mx = int(present.sum()) - 1
    values = []
    for p in planes:
        q = forward[p]
        for j in range(q.shape[2]):
            q[:, :, j] = wav_encode(q[:, :, j], mx)
        values.append(q.reshape(-1))
    values = np.concatenate(values)
    if callable(huf.get("lengths")):
        huf = dict(huf, lengths=huf["lengths"](values))
    block = huf_encode_fast(values) if fast else huf_encode(values, **huf)
    head = struct.pack("<HH", lo, hi) + (stored[lo:hi + 1].tobytes() if lo <= hi else b"")
    return head + struct.pack("<i", len(block)) + block


def decode_chunk(data, width, rows, chan_words):
    """PIZ bytes -> the chunk's scanline bytes; PizError on anything wrong"""
    data = bytes(data)
    if len(data) < 4:
        raise PizError("truncated")
    lo, hi = struct.unpack_from("<HH", data, 0)
    if hi >= 8192:
        raise PizError("maxNonZero")
    bitmap = np.zeros(8192, dtype=np.uint8)
    p = 4
    if lo <= hi:
        if p + hi - lo + 1 > len(data):
            raise PizError("bitmap past the chunk")
        bitmap[lo:hi + 1] = np.frombuffer(data, dtype=np.uint8, count=hi - lo + 1, offset=p)
        p += hi - lo + 1
    if p + 4 > len(data):
        raise PizError("truncated")
    length, = struct.unpack_from("<i", data, p)
    p += 4
    if length < 0 or p + length > len(data):
        raise PizError("length")
    if length == 0:
        raise PizError("no data")
    n_values = width * rows * sum(chan_words)
    values = np.array(huf_decode(data[p:p + length], n_values), dtype=np.int64)
    present = np.unpackbits(bitmap, bitorder="little").astype(bool)
    present[0] = True
    lut = np.zeros(65536, dtype=np.int64)
    idx = np.flatnonzero(present)
    lut[:idx.size] = idx
    mx = idx.size - 1
    rows_out = [[] for _ in range(rows)]
    at = 0
    for w in chan_words:
        q = values[at:at + rows * width * w].reshape(rows, width, w).copy()
        at += rows * width * w
        for j in range(w):
            q[:, :, j] = wav_decode(q[:, :, j], mx)
        q = lut[q].astype("<u2")
        for y in range(rows):
            rows_out[y].append(q[y].tobytes())
    return b"".join(b"".join(r) for r in rows_out)


def raw_rows(channels, names, y0, y1):
    """the scanline bytes of rows y0 .. y1 - 1; channels: {name: (array [h, w], pixel type)}"""
    planes = {n: np.ascontiguousarray(channels[n][0]).astype(exr_ref._DTYPE[channels[n][1]]) for n in names}
    return b"".join(planes[n][y].tobytes() for y in range(y0, y1) for n in names)


def write_exr(path, channels, line_order=exr_ref.INC, origin=(0, 0), chunk_hook=None, compression=PIZ, **enc):
    """a complete single-part scanline PIZ file.  channels: {name: (array [h, w], pixel type)}.  Returns {"row_bytes", "chunks": the
    scanline bytes of each chunk in increasing-y order, "coded", "stored"}.  chunk_hook(c, stored) may replace a chunk's stored bytes."""
    names = sorted(channels)
    h, w = next(iter(channels.values()))[0].shape
    x0, y0 = origin
    types = [(n.encode(), channels[n][1]) for n in names]
    box = struct.pack("<iiii", x0, y0, x0 + w - 1, y0 + h - 1)
    A = exr_ref._attr
    header = (A(b"channels", b"chlist", exr_ref.chlist(types)) + A(b"compression", b"compression", bytes([compression]))
              + A(b"dataWindow", b"box2i", box) + A(b"displayWindow", b"box2i", box)
              + A(b"lineOrder", b"lineOrder", bytes([line_order])) + A(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
              + A(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0))
              + A(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")
    words = [WORDS[channels[n][1]] for n in names]
    chunks, stored, coded = [], [], []
    for c in range(-(-h // LINES)):
        r0, r1 = c * LINES, min(h, (c + 1) * LINES)
        raw = raw_rows(channels, names, r0, r1)
        z = encode_chunk(raw, w, r1 - r0, words, **enc)
        use = z if len(z) < len(raw) else raw
        chunks.append(raw)
        coded.append(use is z)
        stored.append(chunk_hook(c, use) if chunk_hook else use)
    n = len(chunks)
    head = struct.pack("<4sI", b"\x76\x2f\x31\x01", 2) + header
    pos = len(head) + 8 * n
    offsets, body = [0] * n, b""
    for c in (range(n) if line_order == exr_ref.INC else reversed(range(n))):
        offsets[c] = pos + len(body)
        body += struct.pack("<ii", y0 + c * LINES, len(stored[c])) + stored[c]
    with open(path, "wb") as f:
        f.write(head + struct.pack("<%dQ" % n, *offsets) + body)
    return {"row_bytes": len(chunks[0]) // min(h, LINES), "chunks": chunks, "coded": coded, "stored": stored, "words": words}
