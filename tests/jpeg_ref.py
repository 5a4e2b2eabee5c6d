"""Plain Python / NumPy baseline-JPEG decoder: the sequential reference that csrc/jpeg.hip and jpeg.py are tested against, itself
pinned byte for byte against PIL (libjpeg-turbo, islow IDCT, fancy upsampling) by tests/test_jpeg.py.  Stages, each a function:
markers -> unstuffing -> code-by-code Huffman decoding to coefficients -> dequantisation + islow IDCT -> upsampling -> colour.
Written from ITU T.81 and the arithmetic libjpeg documents in jidctint.c / jdsample.c / jdcolor.c; it shares no code with jpeg.py."""
import struct

import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
      56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def markers(data):
    """dict: width, height, comps [(id, h, v, tq, td, ta)], q {id: [64] natural}, huff {(cls, id): (counts, symbols)}, ri,
    scan (start, end), rst [file offsets], orientation"""
    assert data[:2] == b"\xff\xd8"
    out = dict(q={}, huff={}, ri=0, orientation=1)
    pos = 2
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        n, = struct.unpack_from(">H", data, pos + 2)
        seg = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m in (0xC0, 0xC1):
            _, out["height"], out["width"], nc = struct.unpack_from(">BHHB", seg)
            frame = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                wide, t = seg[p] >> 4, seg[p] & 15
                vals = struct.unpack_from(">64H" if wide else "64B", seg, p + 1)
                nat = [0] * 64
                for k in range(64):
                    nat[ZZ[k]] = vals[k]
                out["q"][t] = nat
                p += 129 if wide else 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                counts = list(seg[p + 1:p + 17])
                out["huff"][(seg[p] >> 4, seg[p] & 15)] = (counts, list(seg[p + 17:p + 17 + sum(counts)]))
                p += 17 + sum(counts)
        elif m == 0xDD:
            out["ri"], = struct.unpack(">H", seg)
        elif m == 0xE1 and seg[:6] == b"Exif\0\0":
            t = seg[6:]
            e = "<" if t[:2] == b"II" else ">"
            ifd, = struct.unpack_from(e + "I", t, 4)
            cnt, = struct.unpack_from(e + "H", t, ifd)
            for i in range(cnt):
                tag, _, _, val = struct.unpack_from(e + "HHIH", t, ifd + 2 + 12 * i)
                if tag == 0x0112:
                    out["orientation"] = val
        elif m == 0xDA:
            ns = seg[0]
            sel = {seg[1 + 2 * i]: seg[2 + 2 * i] for i in range(ns)}
            out["comps"] = [(cid, h, v, tq, sel[cid] >> 4, sel[cid] & 15) for cid, h, v, tq in frame]
            break
    start = pos
    rst = []
    while True:
        pos = data.index(b"\xff", pos)
        if data[pos + 1] == 0:
            pos += 2
        elif 0xD0 <= data[pos + 1] <= 0xD7:
            rst.append(pos)
            pos += 2
        else:
            break
    out["scan"], out["rst"] = (start, pos), rst
    return out


def unstuff(data, info):
    """the restart segments as bytes, stuffing removed"""
    cuts = [info["scan"][0]] + [r + 2 for r in info["rst"]]
    ends = info["rst"] + [info["scan"][1]]
    return [data[a:b].replace(b"\xff\x00", b"\xff") for a, b in zip(cuts, ends)]


def code_book(counts, symbols):
    """{(length, code): symbol}"""
    book, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            book[(l, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return book


class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def bit(self):
        byte = self.data[self.pos >> 3]               # IndexError past the end: a damaged stream
        b = (byte >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, book):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            if (l, code) in book:
                return book[(l, code)]
        raise ValueError("no such code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def grid(info):
    """(mcus_x, mcus_y, [(h, v, bw, bh, cw, ch)]) -- a one-component scan is not interleaved: its MCU is one block"""
    w, h = info["width"], info["height"]
    if len(info["comps"]) == 1:
        mx, my = -(-w // 8), -(-h // 8)
        return mx, my, [(1, 1, mx, my, w, h)]
    hmax, vmax = max(c[1] for c in info["comps"]), max(c[2] for c in info["comps"])
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return mx, my, [(ch, cv, mx * ch, my * cv, -(-w * ch // hmax), -(-h * cv // vmax)) for _, ch, cv, _, _, _ in info["comps"]]


def coefficients(data):
    """per component int16 [bh, bw, 64]: quantised coefficients, natural order, DC prediction undone"""
    info = markers(data)
    mx, my, comps = grid(info)
    books = {k: code_book(*v) for k, v in info["huff"].items()}
    coef = [np.zeros((bh, bw, 64), dtype=np.int16) for _, _, bw, bh, _, _ in comps]
    segs = unstuff(data, info)
    ri = info["ri"] or mx * my
    mcu = 0
    for seg in segs:
        bits = _Bits(seg)
        pred = [0] * len(comps)
        for _ in range(min(ri, mx * my - mcu)):
            my_, mx_ = divmod(mcu, mx)
            for c, (h, v, _, _, _, _) in enumerate(comps):
                _, _, _, _, td, ta = info["comps"][c]
                for r in range(h * v):
                    blk = coef[c][my_ * v + r // h, mx_ * h + r % h]
                    s = bits.symbol(books[(0, td)])
                    pred[c] += _extend(bits.bits(s), s)
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(books[(1, ta)])
                        r_, s = rs >> 4, rs & 15
                        if s == 0:
                            if r_ != 15:
                                break
                            k += 16
                            continue
                        k += r_
                        blk[ZZ[k]] = _extend(bits.bits(s), s)
                        k += 1
            mcu += 1
    return info, coef


C = {"298": 2446, "390": 3196, "541": 4433, "765": 6270, "899": 7373, "1175": 9633, "1501": 12299, "1847": 15137, "1961": 16069,
     "2053": 16819, "2562": 20995, "3072": 25172}


def _idct_pass(d, shift):
    """jidctint.c's 1-D pass along axis -2 of int64 [..., 8, n]"""
    z2, z3 = d[..., 2, :], d[..., 6, :]
    z1 = (z2 + z3) * C["541"]
    t2, t3 = z1 - z3 * C["1847"], z1 + z2 * C["765"]
    t0, t1 = (d[..., 0, :] + d[..., 4, :]) << 13, (d[..., 0, :] - d[..., 4, :]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7, :], d[..., 5, :], d[..., 3, :], d[..., 1, :]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * C["1175"]
    t0, t1, t2, t3 = t0 * C["298"], t1 * C["2053"], t2 * C["3072"], t3 * C["1501"]
    z1, z2 = z1 * -C["899"], z2 * -C["2562"]
    z3, z4 = z3 * -C["1961"] + z5, z4 * -C["390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    rows = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(r + (1 << (shift - 1))) >> shift for r in rows], axis=-2)


def planes(info, coef):
    """per component the padded uint8 plane [bh * 8, bw * 8]: dequantise, islow IDCT (columns, then rows), + 128, clamp"""
    out = []
    for c, blocks in enumerate(coef):
        q = np.asarray(info["q"][info["comps"][c][3]], dtype=np.int64)
        d = (blocks.astype(np.int64) * q).reshape(blocks.shape[0], blocks.shape[1], 8, 8)
        d = _idct_pass(d, 11)                                                   # over rows index = columns pass
        d = _idct_pass(d.swapaxes(-1, -2), 18).swapaxes(-1, -2)
        px = np.clip(d + 128, 0, 255).astype(np.uint8)
        out.append(px.transpose(0, 2, 1, 3).reshape(blocks.shape[0] * 8, blocks.shape[1] * 8))
    return out


def upsample(p, hs, vs, cw, ch):
    """chroma plane -> int [ch * vs, cw * hs] as jdsample.c does it on the component's downsampled size cw x ch: h2v2 / h2v1 fancy
    when cw > 2, replication otherwise"""
    p = p[:ch, :cw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)
    if vs == 1:
        left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
        right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
        out = np.empty((ch, 2 * cw), dtype=np.int64)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        return out
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    for par, far in ((0, up), (1, down)):
        col = 3 * p + far                                                       # "thiscolsum" of every column
        left = np.concatenate([col[:, :1], col[:, :-1]], axis=1)
        right = np.concatenate([col[:, 1:], col[:, -1:]], axis=1)
        out[par::2, 0::2] = (3 * col + left + 8) >> 4
        out[par::2, 1::2] = (3 * col + right + 7) >> 4
    return out


def rgb(info, pl):
    w, h = info["width"], info["height"]
    _, _, comps = grid(info)
    y = pl[0][:h, :w].astype(np.int64)
    if len(pl) == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    hs, vs = comps[0][0], comps[0][1]
    cb = upsample(pl[1], hs, vs, comps[1][4], comps[1][5])[:h, :w] - 128
    cr = upsample(pl[2], hs, vs, comps[2][4], comps[2][5])[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data):
    info, coef = coefficients(data)
    return rgb(info, planes(info, coef))


# ---------------------------------------------------------------- test files, written with PIL
SIZES = [(8, 8), (16, 16), (23, 17), (47, 33), (40, 64), (1, 1)]          # (height, width): whole MCUs, partial MCUs of every layout,
LAYOUT_NAMES = ["grey", "444", "422", "420"]                              # planes narrower than libjpeg's fancy upsampler takes
QUALITIES = [30, 75, 100]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def content(seed, h, w, noise=False):
    """uint8 RGB [h, w, 3]: smooth gradients plus mild noise, or pure noise (which at quality 100 gives the longest codes)"""
    rng = np.random.default_rng(seed)
    if noise:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(h + w - 2, 1)], axis=2)
    return np.clip(base + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(img, layout, quality, **kw):
    """JPEG bytes of uint8 RGB `img` in layout "grey" / "444" / "422" / "420" (PIL keywords pass through: optimize,
    restart_marker_blocks, progressive, exif)"""
    import io
    from PIL import Image
    im = Image.fromarray(img)
    if layout == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = SUBSAMPLING[layout]
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=quality, **kw)
    return buf.getvalue()


def pil_rgb(data):
    import io
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def grid_cases():
    """(id, bytes) of the whole grid: every size x layout x quality, an optimised-table file per size, restart intervals of 1 and 3
    blocks on a 4:2:0 and a 4:4:4 file, and one pure-noise image"""
    cases = []
    for si, (h, w) in enumerate(SIZES):
        for layout in LAYOUT_NAMES:
            for q in QUALITIES:
                cases.append(("%dx%d-%s-q%d" % (h, w, layout, q), encode(content(si, h, w, noise=q == 100), layout, q)))
        cases.append(("%dx%d-420-optimize" % (h, w), encode(content(si, h, w), "420", 85, optimize=True)))
    for layout in ("420", "444"):
        for blocks in (1, 3):
            cases.append(("47x33-%s-rst%d" % (layout, blocks), encode(content(7, 47, 33), layout, 75, restart_marker_blocks=blocks)))
    cases.append(("40x64-422-noise-q75", encode(content(9, 40, 64, noise=True), "422", 75)))
    return cases
