"""Baseline-JPEG files built coefficient by coefficient, for the tests of the device decoder (csrc/jpeg.hip, jpeg.py).

encode() writes a file from quantised coefficients, quantisation tables, Huffman tables, sampling factors and a restart interval:
the expected coefficients of a decode are then the writer's INPUT, with no decoder in between, and the expected pixels are PIL's.
That reaches what no encoder emits on its own: tables whose codes are all longer than the decoder's 9-bit look-ahead, one-symbol
tables, four table slots in a scan, DC differences of category 11, blocks without EOB, and streams that never re-synchronise.
Written from ITU T.81; it shares no code with jpeg.py or jpeg_ref.py (only the zig-zag order is imported).

CASES is the fixed list the CPU test (test_jpeg_synth.py) and the device test (test_gpu_jpeg_synth.py) walk.  sync_model()
restates the pass / iteration / carry / flag rules of jpeg_sync_kernel for the all-zero streams and returns the pass count."""
import collections
import functools
import struct

import numpy as np

from jpeg_ref import ZZ

SAMPLING = {"grey": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}


# ---------------------------------------------------------------- the writer
def components(layout, ids=(1, 2, 3), tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1)):
    """[(id, h, v, tq, td, ta)] of a layout name"""
    h, v = SAMPLING[layout]
    first = (ids[0], h, v, tq[0], td[0], ta[0])
    if layout == "grey":
        return [first]
    return [first] + [(ids[c], 1, 1, tq[c], td[c], ta[c]) for c in (1, 2)]


def block_grid(width, height, comps):
    """(mcus_x, mcus_y, [(bh, bw)] per component); a one-component scan is not interleaved: its MCU is one block"""
    if len(comps) == 1:
        mx, my = (width + 7) // 8, (height + 7) // 8
        return mx, my, [(my, mx)]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = (width + 8 * hmax - 1) // (8 * hmax), (height + 8 * vmax - 1) // (8 * vmax)
    return mx, my, [(my * c[2], mx * c[1]) for c in comps]


def _codes(counts, symbols):
    """{symbol: (code, length)}: the canonical codes of T.81 Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code *= 2
    return out


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, n):
        self.acc = (self.acc << n) | value
        self.n += n
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        """pad the last byte with 1-bits, stuff a zero after every FF"""
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out).replace(b"\xff", b"\xff\x00")


def _magnitude(v):
    """(category, the category's extra bits) of a DC difference or an AC value"""
    s = abs(v).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def encode(width, height, comps, coef, qtables, htables, restart_interval=0, wide_q=False, sof=0xC0, adobe=None, extra_segments=(),
           dht_together=False, info=None):
    """bytes of a baseline JPEG file.  comps: [(id, h, v, tq, td, ta)]; coef: per component int [bh, bw, 64], natural order, DC as a
    value; qtables: {id: 64 values, natural order} (wide_q: written as 16-bit); htables: {(class, id): (16 counts, symbols)};
    adobe: the transform byte of an APP14 segment (None: a JFIF APP0 instead); extra_segments: (marker, payload) written before the
    tables; dht_together: all Huffman tables in one DHT segment, not one each; info: a dict that receives scan_start, scan_end and
    rst_offsets (file offsets)."""
    mx, my, grid = block_grid(width, height, comps)
    assert len(coef) == len(comps) and all(tuple(np.shape(a)) == (bh, bw, 64) for a, (bh, bw) in zip(coef, grid))
    out = bytearray(b"\xff\xd8")
    if adobe is None:
        out += _segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    else:
        out += _segment(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe))
    for marker, payload in extra_segments:
        out += _segment(marker, payload)
    for t in sorted(qtables):
        zz = [int(qtables[t][ZZ[k]]) for k in range(64)]
        out += _segment(0xDB, bytes([(16 if wide_q else 0) | t]) + (struct.pack(">64H", *zz) if wide_q else bytes(zz)))
    out += _segment(sof, struct.pack(">BHHB", 8, height, width, len(comps)) + b"".join(bytes([c[0], c[1] << 4 | c[2], c[3]]) for c in comps))
    tables = [bytes([cls << 4 | t]) + bytes(counts) + bytes(symbols) for (cls, t), (counts, symbols) in sorted(htables.items())]
    if dht_together:
        out += _segment(0xC4, b"".join(tables))
    else:
        for t in tables:
            out += _segment(0xC4, t)
    if restart_interval:
        out += _segment(0xDD, struct.pack(">H", restart_interval))
    out += _segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], c[4] << 4 | c[5]]) for c in comps) + b"\0\x3f\0")
    scan_start = len(out)
    dc_codes = [_codes(*htables[(0, c[4])]) for c in comps]
    ac_codes = [_codes(*htables[(1, c[5])]) for c in comps]
    blocks = [np.asarray(a).astype(np.int64)[:, :, ZZ].tolist() for a in coef]                  # zig-zag order, plain ints
    units = [(1, 1)] if len(comps) == 1 else [(c[1], c[2]) for c in comps]
    rst_offsets = []
    bits = _BitWriter()
    pred = [0] * len(comps)
    for mcu in range(mx * my):
        if restart_interval and mcu and mcu % restart_interval == 0:
            out += bits.finish()
            rst_offsets.append(len(out))
            out += bytes([0xFF, 0xD0 + (mcu // restart_interval - 1) % 8])
            bits = _BitWriter()
            pred = [0] * len(comps)
        row, col = divmod(mcu, mx)
        for c, (h, v) in enumerate(units):
            for r in range(h * v):
                zz = blocks[c][row * v + r // h][col * h + r % h]
                s, extra = _magnitude(zz[0] - pred[c])
                pred[c] = zz[0]
                bits.put(*dc_codes[c][s])
                bits.put(extra, s)
                run = 0
                for k in range(1, 64):
                    if zz[k] == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*ac_codes[c][0xF0])
                        run -= 16
                    s, extra = _magnitude(zz[k])
                    bits.put(*ac_codes[c][run << 4 | s])
                    bits.put(extra, s)
                    run = 0
                if run:
                    bits.put(*ac_codes[c][0x00])
    out += bits.finish()
    if info is not None:
        info.update(scan_start=scan_start, scan_end=len(out), rst_offsets=rst_offsets)
    return bytes(out + b"\xff\xd9")


# ---------------------------------------------------------------- Huffman tables
def _ac_symbols():
    """the 162 (run, size) symbols of baseline AC coding, the cheap ones first"""
    pairs = sorted(((run, size) for run in range(16) for size in range(1, 11)), key=lambda rs: (rs[0] + 2 * rs[1], rs[0]))
    syms = [run << 4 | size for run, size in pairs]
    return [0x00] + syms[:3] + [0xF0] + syms[3:]


def _counts(**at):
    """16 counts from l<length>=<count> keywords"""
    counts = [0] * 16
    for k, n in at.items():
        counts[int(k[1:]) - 1] = n
    return counts


DC_TYPICAL = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))                      # the length profile of T.81 table K.3
DC_REVERSED = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(11, -1, -1)))
AC_TYPICAL = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _ac_symbols())                       # the length profile of table K.5
AC_ALL_16 = (_counts(l16=162), sorted(_ac_symbols()))                  # every code has 16 bits: legal, incomplete, no all-ones code
DC_ALL_10 = (_counts(l10=12), list(range(12)))
AC_9_AND_10 = (_counts(l9=81, l10=81), sorted(_ac_symbols()))        # runs 0 ... 7 take 9 bits, runs 8 ... 15 take 10
AC_9_AND_10_MIXED = (_counts(l9=81, l10=81), _ac_symbols()[0::2] + _ac_symbols()[1::2])               # cheap symbols on both sides of the boundary
DC_9_AND_10 = (_counts(l9=6, l10=6), [0, 2, 4, 6, 8, 10, 1, 3, 5, 7, 9, 11])
ONE_SYMBOL = lambda symbol: (_counts(l1=1), [symbol])                  # the single code "0"

TYPICAL = {(0, 0): DC_TYPICAL, (1, 0): AC_TYPICAL, (0, 1): DC_REVERSED, (1, 1): AC_9_AND_10_MIXED}


def flat_q(value):
    return [value] * 64


# ---------------------------------------------------------------- coefficients
def random_coef(seed, grid, density, amp, dc_amp=200):
    """sparse random blocks: each AC nonzero with probability `density`, uniform in +-amp; DC uniform in +-dc_amp"""
    rng = np.random.default_rng(seed)
    out = []
    for bh, bw in grid:
        a = rng.integers(-amp, amp + 1, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < density)
        a[..., 0] = rng.integers(-dc_amp, dc_amp + 1, (bh, bw))
        out.append(a.astype(np.int16))
    return out


def scan_order(bh, bw, h, v):
    """the (row, column) of a component's blocks in the order the scan visits them"""
    return [(my * v + r // h, mx * h + r % h) for my in range(bh // v) for mx in range(bw // h) for r in range(h * v)]


def alternating_dc(grid, comps):
    """DC -1024 / +1023 between consecutive blocks of a component in scan order (differences of +-2047: category 11), no AC"""
    out = []
    for (bh, bw), c in zip(grid, comps):
        a = np.zeros((bh, bw, 64), dtype=np.int16)
        h, v = (1, 1) if len(comps) == 1 else (c[1], c[2])
        for i, (y, x) in enumerate(scan_order(bh, bw, h, v)):
            a[y, x, 0] = 1023 if i % 2 else -1024
        out.append(a)
    return out


def walking_ac(grid, value=1023):
    """one AC of +-value per block, at a zig-zag position that walks over 1 ... 63"""
    out = []
    i = 0
    for bh, bw in grid:
        a = np.zeros((bh, bw, 64), dtype=np.int16)
        for y in range(bh):
            for x in range(bw):
                a[y, x, ZZ[1 + i % 63]] = value if i % 2 else -value
                a[y, x, 0] = (i * 37) % 200 - 100
                i += 1
        out.append(a)
    return out


def last_only(grid):
    """the only AC of every block is the last one of the zig-zag: ZRL, ZRL, ZRL, run 14, and no EOB"""
    out = []
    for n, (bh, bw) in enumerate(grid):
        a = np.zeros((bh, bw, 64), dtype=np.int16)
        a[..., 63] = (np.arange(bh * bw).reshape(bh, bw) % 7) - 3
        a[..., 63][a[..., 63] == 0] = 5 + n
        a[..., 0] = (np.arange(bh * bw).reshape(bh, bw) * 11) % 90 - 45
        out.append(a)
    return out


def dense(seed, grid, amp, every=1):
    """all 63 ACs nonzero, |value| <= amp, in every `every`-th block of a component; the others hold nothing (EOB only, DC difference
    of category 0 after the first)"""
    rng = np.random.default_rng(seed)
    out = []
    for bh, bw in grid:
        mag = rng.integers(1, amp + 1, (bh, bw, 64)) * rng.choice([-1, 1], (bh, bw, 64))
        keep = (np.arange(bh * bw).reshape(bh, bw) % every == 0)[..., None]
        a = mag * keep
        a[..., 0] = 0
        out.append(a.astype(np.int16))
    return out


def every_symbol(grid):
    """every (run, size) of baseline AC coding, ZRL and EOB, and DC differences of every category 0 ... 11, in each component: the
    whole of a Huffman table is used, its last code of every length included.  At most one value of category 10 per block."""
    out = []
    for n, (bh, bw) in enumerate(grid):
        blocks, zz, k, big = [], [0] * 64, 1, False
        pairs = [(run, size) for size in range(1, 11) for run in range(16)]
        pairs = pairs[n * 7:] + pairs[:n * 7]                             # another packing per component
        for i, (run, size) in enumerate(pairs):
            if k + run > 63 or (size == 10 and big):
                blocks.append(zz)
                zz, k, big = [0] * 64, 1, False
            k += run
            zz[k] = ((1 << (size - 1)) + (i * 37) % (1 << (size - 1))) * (-1 if i % 3 == 0 else 1)
            big = big or size == 10
            k += 1
        blocks.append(zz)
        blocks.append([0] * 17 + [3] + [0] * 46)                         # run 16: ZRL + (0, 2), then EOB
        assert len(blocks) <= bh * bw, (len(blocks), bh, bw)
        dc, pred = [], 0
        for s in list(range(12)) + [0]:
            pred += 0 if s == 0 else (1 << (s - 1)) * (1 if s % 2 else -1)
            dc.append(pred)
        a = np.zeros((bh * bw, 64), dtype=np.int16)
        a[:len(blocks)] = np.array(blocks)[:, np.argsort(ZZ)]
        a[:len(dc), 0] = dc
        out.append(a.reshape(bh, bw, 64))
    return out


def constant(grid, values):
    """every AC of component c is values[c], every DC 0"""
    out = []
    for (bh, bw), v in zip(grid, values):
        a = np.full((bh, bw, 64), v, dtype=np.int16)
        a[..., 0] = 0
        out.append(a)
    return out


# ---------------------------------------------------------------- the cases
class Case:
    """name; group ("tables", "coefficients", "restart", "stream", "layout", "refused"); pixels: compared with PIL (False: the named
    extreme cases, coefficients only); args: encode()'s keywords, or None for a file PIL writes (make: () -> bytes); refused: the
    Unsupported message jpeg.plan must raise; zero_stream: bits per block of the MCU of an all-zero stream"""

    def __init__(self, name, group, pixels=True, args=None, make=None, refused=None, zero_stream=None, multi=False):
        self.name, self.group, self.pixels, self.args, self.make, self.refused = name, group, pixels, args, make, refused
        self.zero_stream, self.multi = zero_stream, multi          # multi: decoded at every compiled subsequence length
        self.info = {}

    @functools.cached_property
    def data(self):
        if self.args is None:
            return self.make()
        return encode(info=self.info, **self.args)

    @functools.cached_property
    def coef(self):
        """the expected coefficients: the writer's input; of a PIL-written file the sequential reference's"""
        if self.args is not None:
            return [np.asarray(a, dtype=np.int16) for a in self.args["coef"]]
        import jpeg_ref
        return jpeg_ref.coefficients(self.data)[1]

    @functools.cached_property
    def pil(self):
        import jpeg_ref
        return jpeg_ref.pil_rgb(self.data)

    @property
    def small(self):
        return self.group not in ("stream", "refused")

    def __repr__(self):
        return self.name


def _synth(name, group, width, height, layout, coef, q=(1, 1), tables=None, pixels=True, comp_kw=None, **kw):
    comps = components(layout, **(comp_kw or {}))
    grid = block_grid(width, height, comps)[2]
    tables = TYPICAL if tables is None else tables
    qt = kw.pop("qtables", None) or {0: flat_q(q[0]), 1: flat_q(q[1])}
    extra = {k: kw.pop(k) for k in ("refused", "zero_stream", "multi") if k in kw}
    args = dict(width=width, height=height, comps=comps, coef=coef(grid) if callable(coef) else coef, qtables=qt,
                htables={k: tables[k] for k in sorted({(0, c[4]) for c in comps} | {(1, c[5]) for c in comps})}, **kw)
    return Case(name, group, pixels, args, **extra)


def _pil(name, group, make, **kw):
    return Case(name, group, True, None, make, **kw)


LAYOUT_SIZES = [(1, 3), (2, 4), (1, 5), (2, 6), (3, 3), (5, 1), (17, 1), (1, 17), (2, 2)]           # (height, width)


def _cases():
    import jpeg_ref
    cases = []
    add = lambda *a, **k: cases.append(_synth(*a, **k))
    rnd = lambda seed, density=0.15, amp=40: (lambda grid: random_coef(seed, grid, density, amp))
    # ---- tables
    long_codes = {(0, 0): DC_ALL_10, (1, 0): AC_ALL_16, (0, 1): DC_ALL_10, (1, 1): AC_ALL_16}
    add("huff-all-16-bit-444", "tables", 61, 45, "444", rnd(1, 0.2, 255), tables=long_codes, multi=True)
    add("huff-all-16-bit-420", "tables", 64, 64, "420", rnd(2, 0.3, 100), tables=long_codes, multi=True)
    nine_ten = {(0, 0): DC_9_AND_10, (1, 0): AC_9_AND_10, (0, 1): DC_9_AND_10, (1, 1): AC_9_AND_10_MIXED}
    add("huff-9-10-boundary-420", "tables", 47, 33, "420", rnd(3, 0.25, 500), tables=nine_ten)
    add("huff-9-10-boundary-grey", "tables", 40, 24, "grey", rnd(4, 0.5, 1023), tables=nine_ten)
    add("every-symbol-all-16-bit-grey", "tables", 64, 64, "grey", every_symbol, tables=long_codes)
    add("every-symbol-9-10-boundary-444", "tables", 64, 64, "444", every_symbol, tables=nine_ten)
    add("every-symbol-typical-444", "tables", 64, 64, "444", every_symbol)
    ids23 = {(0, 2): DC_TYPICAL, (1, 2): AC_TYPICAL, (0, 3): DC_9_AND_10, (1, 3): AC_ALL_16}
    add("huff-ids-2-3-422", "tables", 40, 17, "422", rnd(5), tables=ids23, comp_kw=dict(td=(2, 3, 3), ta=(2, 3, 3)))
    four = {(0, 0): DC_TYPICAL, (1, 0): AC_TYPICAL, (1, 1): AC_9_AND_10_MIXED, (1, 2): AC_ALL_16, (0, 1): DC_ALL_10}
    add("huff-four-slots-444", "tables", 24, 24, "444", rnd(6, 0.3), tables=four, comp_kw=dict(td=(0, 0, 0), ta=(0, 1, 2)))
    add("huff-four-slots-420", "tables", 33, 17, "420", rnd(7, 0.3), tables=four, comp_kw=dict(td=(0, 0, 0), ta=(0, 1, 2)))
    add("huff-five-tables-444", "refused", 16, 16, "444", rnd(8), tables=four, comp_kw=dict(td=(0, 1, 1), ta=(0, 1, 2)),
        refused="more than four Huffman tables")
    add("sampling-440", "refused", 16, 16, "440", rnd(9), refused="sampling factors")
    add("dht-one-segment-420", "tables", 24, 40, "420", rnd(10), dht_together=True)
    add("dht-segment-each-420", "tables", 24, 40, "420", rnd(10))
    add("sof1-420", "tables", 31, 31, "420", rnd(11), sof=0xC1)
    add("sof1-grey", "tables", 9, 23, "grey", rnd(12), sof=0xC1)
    sparse3 = lambda seed: (lambda grid: random_coef(seed, grid, 0.04, 3, dc_amp=3))
    add("dqt-16-bit-300-1000-444", "tables", 32, 24, "444", sparse3(13), q=(300, 1000), wide_q=True)
    add("dqt-16-bit-300-1000-420", "tables", 48, 32, "420", sparse3(14), q=(300, 1000), wide_q=True)
    add("dqt-ids-2-3-422", "tables", 35, 20, "422", lambda grid: random_coef(15, grid, 0.15, 6, dc_amp=12), qtables={2: list(range(1, 65)), 3: list(range(64, 0, -1))},
        comp_kw=dict(tq=(2, 3, 3)))
    add("component-ids-0-1-2-420", "tables", 20, 20, "420", rnd(16), comp_kw=dict(ids=(0, 1, 2)))
    add("component-ids-10-20-30-444", "tables", 20, 12, "444", rnd(17), comp_kw=dict(ids=(10, 20, 30)))
    add("adobe-transform-1-444", "tables", 16, 24, "444", rnd(18), adobe=1)
    add("adobe-transform-1-420", "tables", 30, 18, "420", rnd(19), adobe=1)
    add("segments-holding-ff-bytes-422", "tables", 32, 16, "422", rnd(20),
        extra_segments=((0xFE, b"a comment \xff\xd8\xff\xda\x00\x0c\xff\xff\xd9 in it\xff"), (0xE5, b"\xff\xc0\xff\xc4\xff\x00" * 7),
                        (0xEC, bytes(range(200, 256)) * 3)))
    # ---- coefficients (every quantiser 1)
    for layout in ("444", "420", "grey"):
        add("dc-category-11-" + layout, "coefficients", 48, 32, layout,
            lambda grid, layout=layout: alternating_dc(grid, components(layout)))
    add("dc-category-11-restart-1-420", "coefficients", 48, 32, "420", lambda grid: alternating_dc(grid, components("420")),
        restart_interval=1)
    add("dc-category-11-restart-1-444", "coefficients", 24, 16, "444", lambda grid: alternating_dc(grid, components("444")),
        restart_interval=1)
    add("ac-1023-walking-grey", "coefficients", 64, 64, "grey", walking_ac)
    add("ac-1023-walking-422", "coefficients", 64, 32, "422", walking_ac)
    add("ac-1023-walking-all-16-bit-444", "coefficients", 48, 40, "444", walking_ac, tables=long_codes)
    add("only-zigzag-63-420", "coefficients", 33, 33, "420", last_only)
    add("only-zigzag-63-grey", "coefficients", 24, 8, "grey", last_only)
    add("dense-255-444", "coefficients", 24, 16, "444", lambda grid: dense(21, grid, 255))
    add("dense-255-420", "coefficients", 32, 32, "420", lambda grid: dense(22, grid, 255))
    add("dense-next-to-eob-only-420", "coefficients", 48, 32, "420", lambda grid: dense(23, grid, 255, every=2))
    add("dense-next-to-eob-only-grey", "coefficients", 40, 24, "grey", lambda grid: dense(24, grid, 255, every=3))
    # the two extreme cases: their dequantised values leave what an encoder produces (libjpeg-turbo's 16-bit IDCT overflows)
    add("extreme-dense-1023-444", "coefficients", 24, 24, "444", lambda grid: dense(25, grid, 1023), pixels=False)
    add("extreme-dqt-65535-grey", "coefficients", 32, 16, "grey", lambda grid: random_coef(26, grid, 0.3, 1, dc_amp=1), q=(65535, 65535),
        wide_q=True, pixels=False)
    # ---- restart intervals (56 x 40 in 4:2:0: 4 x 3 MCUs)
    add("restart-splits-the-mcu-row-420", "restart", 56, 40, "420", rnd(30, 0.3), restart_interval=3)
    add("restart-splits-the-mcu-row-422", "restart", 56, 40, "422", rnd(31, 0.3), restart_interval=3)
    add("restart-equals-the-mcus-420", "restart", 56, 40, "420", rnd(32, 0.3), restart_interval=12)
    add("restart-larger-than-the-mcus-420", "restart", 56, 40, "420", rnd(33, 0.3), restart_interval=100)
    add("restart-15-segments-444", "restart", 40, 24, "444", rnd(34, 0.3), restart_interval=1)      # RSTn wraps around
    add("restart-35-segments-grey", "restart", 56, 40, "grey", rnd(35, 0.3), restart_interval=1)
    # ---- streams of zero bits: one-symbol tables (the code "0"), every DC 0, every AC -1 / -3 / -7.  A symbol reads the same from
    # any bit position, so a decoder on a wrong phase never meets the true chain: the synchronisation is a sequential chain
    one = {(0, 0): ONE_SYMBOL(0), (1, 0): ONE_SYMBOL(0x01), (1, 1): ONE_SYMBOL(0x02), (1, 2): ONE_SYMBOL(0x03)}
    zero_kw = dict(tables=one, comp_kw=dict(td=(0, 0, 0), ta=(0, 1, 2)), multi=True)
    add("zeros-422", "stream", 384, 128, "422", lambda grid: constant(grid, (-1, -3, -7)), zero_stream=(127, 127, 190, 253), **zero_kw)
    add("zeros-420", "stream", 384, 256, "420", lambda grid: constant(grid, (-1, -3, -7)), zero_stream=(127,) * 4 + (190, 253), **zero_kw)
    add("zeros-grey", "stream", 512, 384, "grey", lambda grid: constant(grid, (-1,)), zero_stream=(127,), **zero_kw)
    # ---- periodic real-world streams and segments that straddle workgroups, written by PIL
    flat = lambda level: (lambda: jpeg_ref.encode(np.full((1024, 2048, 3), level, dtype=np.uint8), "grey", 90))
    cases.append(_pil("flat-white-1024x2048-grey", "stream", flat(255), multi=True))
    cases.append(_pil("flat-mid-grey-1024x2048-grey", "stream", flat(128), multi=True))
    cases.append(_pil("noise-256x384-restart-40-420", "stream",
                      lambda: jpeg_ref.encode(jpeg_ref.content(11, 256, 384, noise=True), "420", 95, restart_marker_blocks=40), multi=True))
    # ---- layout edges: chroma planes 1, 2 and 3 wide (libjpeg replicates up to 2 and interpolates from 3), 1 and 2 high
    for n, (h, w) in enumerate(LAYOUT_SIZES):
        for layout in ("422", "420") + (("grey",) if w == 1 else ()):
            for kind, quality in (("smooth", 90), ("noise", 100)):
                make = lambda n=n, h=h, w=w, layout=layout, kind=kind, quality=quality: jpeg_ref.encode(
                    jpeg_ref.content(40 + n, h, w, noise=kind == "noise"), layout, quality)
                cases.append(_pil("%dx%d-%s-%s" % (h, w, layout, kind), "layout", make))
    return cases


EXTREME = ("extreme-dense-1023-444", "extreme-dqt-65535-grey")                                     # the only cases without pixels
CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES) and tuple(c.name for c in CASES if not c.pixels) == EXTREME


# ---------------------------------------------------------------- jpeg_sync_kernel on an all-zero stream
WG = 256
Sync = collections.namedtuple("Sync", "passes workgroups iterations rounds")


def _symbol_starts(block_bits):
    """bit offsets in the MCU at which a symbol starts (a DC symbol of 1 bit, then 63 AC symbols of equal length per block), the
    block each belongs to, and the bits of an MCU"""
    starts, block, o = [], [], 0
    for b, bits in enumerate(block_bits):
        assert (bits - 1) % 63 == 0
        for k in range(64):
            starts.append(o)
            block.append(b)
            o += 1 if k == 0 else (bits - 1) // 63
    return np.array(starts, dtype=np.int64), np.array(block, dtype=np.int64), o


def _sequential_walk(block_bits, n_mcus, subseq_bits):
    """symbol by symbol through the whole stream: per subsequence the (bit position, symbol of the MCU) where the first symbol at or
    after its end starts"""
    lengths = [1 if k == 0 else (bits - 1) // 63 for bits in block_bits for k in range(64)]
    total = n_mcus * sum(lengths)
    ends = [min(e, total) for e in range(subseq_bits, total + subseq_bits, subseq_bits)]
    out, p, i, k = [], 0, 0, 0
    while k < len(ends):
        if p >= ends[k]:
            out.append((p, i))
            k += 1
            continue
        p += lengths[i]
        i = i + 1 if i + 1 < len(lengths) else 0
    return out


def sync_model(block_bits, n_mcus, subseq_bits, detail=False):
    """the number of launches of jpeg_sync_kernel (csrc/jpeg.hip) on a one-segment stream of zero bits whose MCU has blocks of
    `block_bits` bits.  The kernel's rules restated: pass 0 decodes every subsequence from the assumed state; in a pass the
    workgroup iterates (at most WG + 1 times) while a thread whose left neighbour's end state differs from the state it last
    started from decodes again; thread 0 reads the carry the previous pass wrote; a pass whose last end state of some workgroup
    differs from the previous pass's sets the flag, and the host launches passes until one leaves the flag clear (one workgroup:
    two passes).  A decode is a closed form here: the symbol lengths of such a stream depend on the decoder's state alone.
    Asserts that the final states are those of a sequential walk.  detail: Sync(passes, workgroups, iterations per pass (the
    largest of its workgroups), per subsequence the round pass * (WG + 2) + iteration of its last change)."""
    starts, _, mcu_bits = _symbol_starts(block_bits)
    total = n_mcus * mcu_bits
    assert total % 8 == 0, "the model has no padding bits"
    n_sub = -(-total // subseq_bits)
    nwg = -(-n_sub // WG)
    g = np.arange(nwg * WG, dtype=np.int64)
    valid, first = g < n_sub, g == 0
    p0 = g * subseq_bits
    end = np.minimum(p0 + subseq_bits, total)
    pack = lambda p, i: p * 1024 + i

    def run(state, end):
        """decode from `state` until the bit position reaches `end`: the packed state of the first symbol start at or after it"""
        p, i = state // 1024, state % 1024
        origin = p - starts[i]                                            # where the decoder believes an MCU starts
        x = np.maximum(end, p) - origin
        k, r = x // mcu_bits, x % mcu_bits
        j = np.searchsorted(starts, r, side="left")
        wrap = j == starts.size
        return pack(origin + (k + wrap) * mcu_bits + np.where(wrap, 0, starts[np.minimum(j, starts.size - 1)]), np.where(wrap, 0, j))

    assumed = pack(p0, 0)
    state, last_in, rounds = np.zeros_like(g), assumed.copy(), np.zeros_like(g)
    carry = np.zeros((2, nwg), dtype=np.int64)
    passes, iterations = 0, []
    for pas in range(nwg + 2):
        par, flag, most = pas & 1, False, 0
        for wg in range(nwg):
            sl = slice(wg * WG, (wg + 1) * WG)
            if pas == 0:
                st, mine = np.where(valid[sl], run(assumed[sl], end[sl]), 0), assumed[sl].copy()
            else:
                st, mine = state[sl].copy(), last_in[sl].copy()
            carry_in = carry[par ^ 1, wg - 1] if pas > 0 and wg > 0 else assumed[sl][0]
            when = rounds[sl].copy()
            for it in range(1, WG + 2):
                inn = np.concatenate([[carry_in], st[:-1]])
                need = valid[sl] & ~first[sl] & (inn != mine)
                out = np.where(need, run(inn, end[sl]), st)
                mine = np.where(need, inn, mine)
                changed = need & (out != st)
                st = np.where(changed, out, st)
                when[changed] = pas * (WG + 2) + it
                if not changed.any():
                    break
            most = max(most, it)
            state[sl], last_in[sl], rounds[sl] = st, mine, when
            carry[par, wg] = st[-1]
            if pas > 0 and st[-1] != carry[par ^ 1, wg]:
                flag = True
        passes += 1
        iterations.append(most)
        if pas == 0:
            continue
        if nwg == 1 or not flag:
            break
    walk = _sequential_walk(block_bits, n_mcus, subseq_bits)
    assert len(walk) == n_sub and [(int(s) // 1024, int(s) % 1024) for s in state[:n_sub]] == walk, "the model left the sequential chain"
    return Sync(passes, nwg, iterations, np.where(valid, rounds, -1)) if detail else passes
