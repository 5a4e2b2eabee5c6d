"""An independent NumPy writer of baseline-JPEG files, the reference of the encoder tests (test_jpeg_enc_host.py,
test_gpu_jpeg_enc.py).  It shares no code with csrc/jpeg_enc.h: the forward maths is oracle/camera.py's restatement of libjpeg
(colour conversion constants, islow FDCT, IJG quantiser), the edge rules are written out here on whole planes, the scan is
jpeg_synth.encode's (taken through info=), and the header is composed here because PIL orders the DHT segments DC0, AC0, DC1, AC1
while jpeg_synth sorts them by (class, id).  encode() is held byte-equal to PIL by test_jpeg_enc_host.py.

Also here: the Annex-K Huffman tables as jpeg_synth takes them (STANDARD), arena() -- per-component coefficient arrays to the encoder's
int16 [blocks, 64] arena (zig-zag order, MCU scan order) -- and the coefficient cases of the entropy-stage tests."""
import struct

import numpy as np

import jpeg_synth
from jpeg_ref import ZZ
from oracle import camera as ocam

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}                        # PIL's keyword

_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
STANDARD = {(0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
            (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(_AC_LUMA)),
            (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
            (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(_AC_CHROMA))}
assert len(_AC_LUMA) == len(_AC_CHROMA) == 162 and all(sum(c) == len(s) for c, s in STANDARD.values())


def _fdct_quant(plane, q):
    """[8 bh, 8 bw] samples -> quantised coefficients int64 [bh, bw, 64], natural order"""
    b = ocam._blocks(plane.astype(np.int64) - 128)
    c = ocam._fdct_pass(b, True)
    c = ocam._fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)
    q8 = q.astype(np.int64)[None, None] * 8
    out = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)
    return out.reshape(out.shape[0], out.shape[1], 64)


def _edge(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def coefficients(rgb, layout, quality):
    """(comps, per component the quantised coefficients [bh, bw, 64] over the MCU grid, dummy blocks included) of uint8 [H, W, 3]"""
    rgb = np.asarray(rgb).astype(np.int64)
    height, width, _ = rgb.shape
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    half, off = 1 << 15, 128 << 16
    fx = ocam._fix16
    y = (fx(0.29900) * r + fx(0.58700) * g + fx(0.11400) * b + half) >> 16
    cb = (-fx(0.16874) * r - fx(0.33126) * g + fx(0.50000) * b + off + half - 1) >> 16
    cr = (fx(0.50000) * r - fx(0.41869) * g - fx(0.08131) * b + off + half - 1) >> 16
    comps = jpeg_synth.components(layout)
    h, v = jpeg_synth.SAMPLING[layout]
    mx, my, grid = jpeg_synth.block_grid(width, height, comps)
    ql, qc = ocam.quant_tables(quality)
    # Y: the blocks that hold image samples, from the plane replicated to whole blocks
    ybh, ybw = -(-height // 8), -(-width // 8)
    cy = np.zeros((my * v, mx * h, 64), dtype=np.int64)
    cy[:ybh, :ybw] = _fdct_quant(_edge(y, 8 * ybh, 8 * ybw), ql)
    # its dummy blocks: no AC, the DC of the block before them in the MCU (a dummy row starts from the last block of the row above)
    for row in range(my):
        for col in range(mx):
            prev = None
            for k in range(h * v):
                by, bx = row * v + k // h, col * h + k % h
                if by >= ybh or bx >= ybw:
                    cy[by, bx, 0] = prev
                prev = cy[by, bx, 0]
    out = [cy]
    cbh, cbw = grid[1]
    for plane in (cb, cr):
        # replicated to the right at full resolution up to the block grid, downwards only up to a multiple of v ...
        full = _edge(plane, -(-height // v) * v, 8 * cbw * h)
        if (h, v) == (2, 2):
            s = full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]
            down = (s + (1 + (np.arange(s.shape[1]) & 1))[None, :]) >> 2
        elif (h, v) == (2, 1):
            s = full[:, 0::2] + full[:, 1::2]
            down = (s + (np.arange(s.shape[1]) & 1)[None, :]) >> 1
        else:
            down = full
        # ... and the DOWNSAMPLED rows replicated to the block grid
        out.append(_fdct_quant(_edge(down, 8 * cbh, 8 * cbw), qc))
    return comps, out


def header(width, height, layout, quality, restart_interval=0):
    """SOI ... SOS as PIL writes them"""
    seg = lambda marker, payload: bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)
    h, v = jpeg_synth.SAMPLING[layout]
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for t, q in enumerate(ocam.quant_tables(quality)):
        out += seg(0xDB, bytes([t]) + bytes(int(q.reshape(64)[ZZ[k]]) for k in range(64)))
    out += seg(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, h << 4 | v, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for cls, t in ((0, 0), (1, 0), (0, 1), (1, 1)):
        counts, symbols = STANDARD[(cls, t)]
        out += seg(0xC4, bytes([cls << 4 | t]) + bytes(counts) + bytes(symbols))
    if restart_interval:
        out += seg(0xDD, struct.pack(">H", restart_interval))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def scan(width, height, layout, coef, restart_interval=0):
    """the entropy-coded scan (stuffed segments, RSTn markers between them) of per-component coefficients [bh, bw, 64], natural order,
    with the standard tables: jpeg_synth.encode's"""
    info = {}
    data = jpeg_synth.encode(width, height, jpeg_synth.components(layout), coef, {0: jpeg_synth.flat_q(1), 1: jpeg_synth.flat_q(1)}, STANDARD,
                             restart_interval=restart_interval, info=info)
    return data[info["scan_start"]:info["scan_end"]]


def encode(rgb, layout, quality, restart_interval=0):
    """the complete file"""
    height, width, _ = np.shape(rgb)
    _, coef = coefficients(rgb, layout, quality)
    return header(width, height, layout, quality, restart_interval) + scan(width, height, layout, coef, restart_interval) + b"\xff\xd9"


def pil_encode(rgb, layout, quality, restart_interval=0):
    import io
    from PIL import Image
    buf = io.BytesIO()
    kw = dict(restart_marker_blocks=restart_interval) if restart_interval else {}
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[layout], **kw)
    return buf.getvalue()


def arena(width, height, layout, coef):
    """per-component coefficients [bh, bw, 64] (natural order) -> int16 [blocks, 64]: MCU after MCU, Y blocks row-major in the MCU, then
    Cb, Cr; zig-zag order"""
    comps = jpeg_synth.components(layout)
    mx, my, grid = jpeg_synth.block_grid(width, height, comps)
    blocks = []
    for row in range(my):
        for col in range(mx):
            for c, comp in enumerate(comps):
                h, v = comp[1], comp[2]
                for k in range(h * v):
                    blocks.append(np.asarray(coef[c][row * v + k // h, col * h + k % h])[ZZ])
    return np.ascontiguousarray(np.array(blocks, dtype=np.int16))


# ---------------------------------------------------------------- the test grid
SIZES = [(1, 1), (2, 2), (6, 6), (8, 8), (10, 12), (12, 3), (3, 12), (16, 16), (7, 9), (17, 33), (23, 17), (24, 40), (40, 24), (9, 40),
         (33, 8), (48, 64)]                                        # (H, W)
QUALITIES = [1, 10, 30, 50, 75, 90, 100]
LAYOUTS = ["444", "422", "420"]
CONTENTS = ["noise", "ramp", "black", "white"]


def content(kind, height, width, seed=0):
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)
    if kind == "ramp":
        yy, xx = np.mgrid[0:height, 0:width]
        return np.stack([xx * 255 // max(width - 1, 1), yy * 255 // max(height - 1, 1), (xx + yy) * 255 // max(height + width - 2, 1)],
                        axis=2).astype(np.uint8)
    return np.full((height, width, 3), 0 if kind == "black" else 255, dtype=np.uint8)


def mcu_grid(height, width, layout):
    h, v = jpeg_synth.SAMPLING[layout]
    return -(-width // (8 * h)), -(-height // (8 * v))


def restart_intervals(height, width, layout):
    """0, 1, 2, one larger than an MCU row, one >= the MCU count"""
    mx, my = mcu_grid(height, width, layout)
    return [0, 1, 2, mx + 1, mx * my + 3]


# ---------------------------------------------------------------- coefficient cases of the entropy stage
def coefficient_cases():
    """[(name, width, height, layout, restart interval, per-component coefficients)]: jpeg_synth's generators on the standard tables"""
    S = jpeg_synth
    cases = []

    def add(name, width, height, layout, restart, make):
        comps = S.components(layout)
        grid = S.block_grid(width, height, comps)[2]
        cases.append((name, width, height, layout, restart, make(grid, comps)))
    add("random-444", 61, 45, "444", 0, lambda g, c: S.random_coef(1, g, 0.2, 255))
    add("random-420-restart-3", 56, 40, "420", 3, lambda g, c: S.random_coef(2, g, 0.3, 100))
    add("random-422-restart-1", 40, 17, "422", 1, lambda g, c: S.random_coef(3, g, 0.15, 40))
    add("dense-255-420", 32, 32, "420", 0, lambda g, c: S.dense(22, g, 255))
    add("dense-next-to-eob-only-444", 48, 32, "444", 2, lambda g, c: S.dense(23, g, 255, every=2))
    add("every-symbol-444", 64, 64, "444", 0, lambda g, c: S.every_symbol(g))
    add("walking-ac-1023-422", 64, 32, "422", 0, lambda g, c: S.walking_ac(g, 1023))
    add("last-only-420", 33, 33, "420", 5, lambda g, c: S.last_only(g))
    add("alternating-dc-420-restart-1", 48, 32, "420", 1, lambda g, c: S.alternating_dc(g, c))
    add("alternating-dc-444", 48, 32, "444", 0, lambda g, c: S.alternating_dc(g, c))
    add("constant-1023-444", 40, 24, "444", 4, lambda g, c: S.constant(g, (1023, 1023, 1023)))            # the stuffing case: runs of 1-bits
    add("constant-minus-1-422", 24, 24, "422", 0, lambda g, c: S.constant(g, (-1, -3, -7)))
    return cases
