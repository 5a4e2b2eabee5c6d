"""CPU tests of the OpenEXR reader (exr.py): the header and payload of a hand-assembled file, the predictor / interleave on a
hand-computed case, every refusal, the host RLE decoder, and read_payload on files of every compression and line order written
by the tests' own writer (exr_ref.py).  The device side: tests/test_gpu_exr.py."""
import ctypes
import importlib
import os
import struct
import zlib

import numpy as np
import pytest

import exr_ref as X

pkg = importlib.import_module("singlehdr-tf2_amd")
E = pkg.exr
D = pkg.dataset


# --- a 3 x 2 NO_COMPRESSION file, assembled byte by byte -----------------------------------------------------------
def _known_file():
    """channels B (HALF), G (FLOAT), R (HALF); data window (-1, 5) - (1, 6); one scanline per chunk"""
    def attr(name, atype, value):
        return name + b"\0" + atype + b"\0" + struct.pack("<i", len(value)) + value
    chl = (b"B\0" + struct.pack("<iB3xii", 1, 0, 1, 1) + b"G\0" + struct.pack("<iB3xii", 2, 0, 1, 1)
           + b"R\0" + struct.pack("<iB3xii", 1, 0, 1, 1) + b"\0")
    header = (b"\x76\x2f\x31\x01" + b"\x02\x00\x00\x00"
              + attr(b"channels", b"chlist", chl)
              + attr(b"compression", b"compression", b"\x00")
              + attr(b"dataWindow", b"box2i", struct.pack("<iiii", -1, 5, 1, 6))
              + attr(b"displayWindow", b"box2i", struct.pack("<iiii", 0, 0, 9, 9))
              + attr(b"lineOrder", b"lineOrder", b"\x00")
              + attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
              + attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0))
              + attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")
    # row 0: B = 1, 2, 0.5  G = 0.25, -3, 100  R = 0, -1, 65504;  row 1: B = -0, 0.5, 1  G = 7, 8, 9  R = 2, 2, 2
    row0 = (bytes.fromhex("003c 0040 0038".replace(" ", "")) + struct.pack("<3f", 0.25, -3.0, 100.0)
            + bytes.fromhex("0000 00bc ff7b".replace(" ", "")))
    row1 = (bytes.fromhex("0080 0038 003c".replace(" ", "")) + struct.pack("<3f", 7.0, 8.0, 9.0)
            + bytes.fromhex("0040 0040 0040".replace(" ", "")))
    table_at = len(header)
    c0 = table_at + 16
    c1 = c0 + 8 + 24
    data = header + struct.pack("<QQ", c0, c1) + struct.pack("<ii", 5, 24) + row0 + struct.pack("<ii", 6, 24) + row1
    rgb = np.array([[[0, 0.25, 1], [-1, -3, 2], [65504, 100, 0.5]], [[2, 7, -0.0], [2, 8, 0.5], [2, 9, 1]]], dtype=np.float32)
    return data, table_at, row0 + row1, rgb


KNOWN_RGB = _known_file()[3]


def known_file(tmp_path):
    data, table_at, planes, rgb = _known_file()
    path = str(tmp_path / "known.exr")
    open(path, "wb").write(data)
    return path, table_at, planes


def test_known_header_and_payload(tmp_path):
    path, table_at, planes = known_file(tmp_path)
    h = E.read_header(path)
    assert h.data_window == (-1, 5, 1, 6) and (h.width, h.height) == (3, 2)
    assert h.channels == (E.Channel("B", E.HALF, 0), E.Channel("G", E.FLOAT, 6), E.Channel("R", E.HALF, 18))
    assert h.compression == E.NO_COMPRESSION and h.line_order == E.INCREASING_Y
    assert (h.lines, h.row_bytes, h.n_chunks, h.table_offset) == (1, 24, 2, table_at)
    p = E.read_payload(path)
    assert p.data.tobytes() == planes
    assert p.offsets.tolist() == [0, 24, 48] and p.coded.tolist() == [0, 0]
    assert E.is_exr(path)
    assert E.channel_table(h, "BGR") == ([0, 6, 18], [E.HALF, E.FLOAT, E.HALF])


def test_predictor_known_answer():
    raw = bytes([10, 20, 30, 40, 250, 3, 7])
    # interleave: even bytes 10 30 250 7, then odd bytes 20 40 3 -> t = 10 30 250 7 20 40 3
    # delta: 10, 30-10+128, 250-30+128, 7-250+128, 20-7+128, 40-20+128, 3-40+128 (mod 256)
    coded = bytes([10, 148, 92, 141, 141, 148, 91])
    assert X.predict(raw) == coded
    assert X.unpredict(coded) == raw
    assert X.unpredict(X.predict(b"\x05")) == b"\x05" and X.unpredict(b"") == b""


# --- refusals ------------------------------------------------------------------------------------------------------
def _image(h, w, seed=0):
    rng = np.random.default_rng(seed)
    img = rng.normal(0.0, 2.0, (h, w)).astype(np.float32)
    img[:, : w // 2] = 1.5                                       # flat half: compresses
    return img


def _rgb_channels(h=20, w=9, t=X.HALF, extra=None):
    ch = {c: (_image(h, w, i), t) for i, c in enumerate("RGB")}
    ch.update(extra or {})
    return ch


def _patch(path, at, new):
    data = bytearray(open(path, "rb").read())
    data[at:at + len(new)] = new
    open(path, "wb").write(bytes(data))


def _refused(path, *words):
    with pytest.raises(ValueError) as info:
        E.read_payload(path)
    msg = str(info.value)
    assert os.path.basename(path) in msg, msg
    for w in words:
        assert w in msg, msg
    return msg


@pytest.mark.parametrize("flag,word", [(0x200, "tiled"), (0x800, "deep"), (0x1000, "multi-part")])
def test_refuses_tiled_deep_multipart(tmp_path, flag, word):
    path = str(tmp_path / ("f%x.exr" % flag))
    X.write_exr(path, _rgb_channels(), X.ZIP, version_flags=flag)
    _refused(path, word)
    with pytest.raises(ValueError, match=word):
        E.read_header(path)


def test_long_names_flag_is_accepted(tmp_path):
    path = str(tmp_path / "long.exr")
    X.write_exr(path, _rgb_channels(extra={"a.very.long.channel.name.beyond.31.bytes": (_image(20, 9), X.FLOAT)}), X.ZIP,
                version_flags=0x400)
    assert E.read_header(path).channels[0].name == "B"
    short = str(tmp_path / "short.exr")
    X.write_exr(short, _rgb_channels(extra={"a.very.long.channel.name.beyond.31.bytes": (_image(20, 9), X.FLOAT)}), X.ZIP)
    _refused(short, "longer than 31")


@pytest.mark.parametrize("code,name", [(4, "PIZ"), (5, "PXR24"), (6, "B44"), (7, "B44A"), (8, "DWAA"), (9, "DWAB")])
def test_refuses_other_compressions(tmp_path, code, name):
    path = str(tmp_path / ("c%d.exr" % code))
    X.write_exr(path, _rgb_channels(), X.ZIP)
    data = open(path, "rb").read()
    at = data.index(b"compression\0compression\0") + len(b"compression\0compression\0") + 4
    _patch(path, at, bytes([code]))
    assert _refused(path, "compression").split(": ", 1)[1].startswith(name + " ")


def test_refuses_missing_colour_channels(tmp_path):
    path = str(tmp_path / "gb.exr")
    X.write_exr(path, {"G": (_image(4, 4), X.HALF), "B": (_image(4, 4), X.HALF), "A": (_image(4, 4), X.HALF)}, X.ZIP)
    _refused(path, "no R channel")
    path = str(tmp_path / "yc.exr")                                  # luminance / chroma
    X.write_exr(path, {"Y": (_image(4, 4), X.HALF), "RY": (_image(4, 4), X.HALF), "BY": (_image(4, 4), X.HALF)}, X.ZIP)
    _refused(path, "no R channel", "luminance")


def test_refuses_uint_colour_and_sampling(tmp_path):
    path = str(tmp_path / "u.exr")
    ch = _rgb_channels()
    ch["G"] = (np.arange(180, dtype=np.uint32).reshape(20, 9), X.UINT)
    X.write_exr(path, ch, X.NONE)
    _refused(path, "channel G is UINT")
    path = str(tmp_path / "s.exr")
    X.write_exr(path, _rgb_channels(extra={"A": (_image(20, 9), X.HALF)}), X.NONE, sampling={b"A": (2, 2)})
    _refused(path, "'A'", "sampling 2 x 2")


@pytest.mark.parametrize("window", [(0, 0, -1, 5), (3, 3, 3, 2), (0, 0, (1 << 20), 0), (-(1 << 30), 0, 1 << 30, 0)])
def test_refuses_empty_or_absurd_window(tmp_path, window):
    path = str(tmp_path / "w.exr")
    X.write_exr(path, _rgb_channels(), X.NONE)
    data = open(path, "rb").read()
    at = data.index(b"dataWindow\0box2i\0") + len(b"dataWindow\0box2i\0") + 4
    _patch(path, at, struct.pack("<iiii", *window))
    _refused(path, "data window", "empty or absurd")


def test_refuses_random_line_order(tmp_path):
    path = str(tmp_path / "r.exr")
    X.write_exr(path, _rgb_channels(), X.ZIPS)
    data = open(path, "rb").read()
    _patch(path, data.index(b"lineOrder\0lineOrder\0") + len(b"lineOrder\0lineOrder\0") + 4, b"\x02")
    _refused(path, "line order 2")


def test_refuses_truncated_header_and_table(tmp_path):
    path = str(tmp_path / "t.exr")
    info = X.write_exr(path, _rgb_channels(), X.ZIPS)
    data = open(path, "rb").read()
    cut = str(tmp_path / "cut.exr")
    for n in (3, 7, 30, 200, info["table_at"] - 1):
        open(cut, "wb").write(data[:n])
        _refused(cut, "truncated header")
    for n in (info["table_at"], info["table_at"] + 8 * 20 - 1):
        open(cut, "wb").write(data[:n])
        _refused(cut, "truncated offset table")
    open(cut, "wb").write(data[:info["table_at"] + 8 * 20 + 5])
    _refused(cut, "chunk")


def test_refuses_bad_chunk_offsets_sizes_and_y(tmp_path):
    path = str(tmp_path / "o.exr")
    info = X.write_exr(path, _rgb_channels(), X.ZIP)
    t = info["table_at"]
    size = os.path.getsize(path)
    _patch(path, t + 8, struct.pack("<Q", size - 4))
    _refused(path, "chunk 1", "outside")
    X.write_exr(path, _rgb_channels(), X.ZIP)
    _patch(path, t, struct.pack("<Q", 3))                            # into the header
    _refused(path, "chunk 0", "outside")
    X.write_exr(path, _rgb_channels(), X.ZIP)
    _patch(path, info["offsets"][1] + 4, struct.pack("<i", size))
    _refused(path, "chunk 1", "past the end")
    X.write_exr(path, _rgb_channels(), X.ZIP)
    _patch(path, info["offsets"][1] + 4, struct.pack("<i", -5))
    _refused(path, "chunk 1", "size -5")
    X.write_exr(path, _rgb_channels(), X.ZIP)
    _patch(path, info["offsets"][1], struct.pack("<i", 0))          # y of chunk 1 must be 16
    _refused(path, "chunk 1", "y is 0", "implies 16")


def test_refuses_bad_chunk_data(tmp_path):
    path = str(tmp_path / "d.exr")
    raw = 20 * 9 * 3 * 2 // 2                                           # ZIPS: one scanline of 3 HALF channels is 54 bytes
    X.write_exr(path, _rgb_channels(), X.ZIPS, chunk_hook=lambda c, z: zlib.compress(bytes(53)) if c == 4 else z)
    _refused(path, "chunk 4", "decodes to 53 bytes", "hold 54")
    X.write_exr(path, _rgb_channels(), X.ZIPS, chunk_hook=lambda c, z: zlib.compress(bytes(900))[:50] if c == 2 else z)
    _refused(path, "chunk 2", "more than 54")
    X.write_exr(path, _rgb_channels(), X.ZIPS, chunk_hook=lambda c, z: b"\x78\x9c\xff\xff\xff\x00" if c == 3 else z)
    _refused(path, "chunk 3", "zlib error")
    X.write_exr(path, _rgb_channels(), X.ZIPS, chunk_hook=lambda c, z: zlib.compress(bytes(54))[:-3] if c == 3 else z)
    _refused(path, "chunk 3", "zlib error")
    X.write_exr(path, _rgb_channels(), X.NONE, chunk_hook=lambda c, z: z[:-2] if c == 7 else z)
    _refused(path, "chunk 7", "52 bytes stored")
    X.write_exr(path, _rgb_channels(), X.ZIPS, chunk_hook=lambda c, z: z + bytes(60) if c == 1 else z)
    _refused(path, "chunk 1", "114 bytes stored")
    X.write_exr(path, _rgb_channels(), X.RLE, chunk_hook=lambda c, z: bytes([127, 1]) if c == 0 else z)
    _refused(path, "chunk 0", "overruns the output")
    X.write_exr(path, _rgb_channels(), X.RLE, chunk_hook=lambda c, z: bytes([20, 1, 256 - 40]) + bytes(10) if c == 0 else z)
    _refused(path, "chunk 0", "overruns the input")
    X.write_exr(path, _rgb_channels(), X.RLE, chunk_hook=lambda c, z: bytes([20, 1]) if c == 0 else z)
    _refused(path, "chunk 0", "decodes to 21 bytes")
    assert raw == 540


# --- host RLE decoder ----------------------------------------------------------------------------------------------
def _rle(data, capacity):
    src = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)          # + 1: a pointer even for empty input
    out = np.full(capacity + 16, 0xEE, dtype=np.uint8)
    lib = pkg._lib.load()
    n = lib.shdr_exr_rle_decode(ctypes.c_void_p(src.ctypes.data), len(data), ctypes.c_void_p(out.ctypes.data), capacity)
    assert (out[capacity:] == 0xEE).all(), "wrote past capacity"
    return n, out[:max(n, 0)].tobytes()


def _rle_numpy(b):
    """the decode rule on an int8 view: c < 0 -> -c literals; else c + 1 copies"""
    out, i, s = [], 0, np.frombuffer(bytes(b), dtype=np.int8)
    while i < len(s):
        c = int(s[i])
        if c < 0:
            out.append(np.frombuffer(bytes(b), dtype=np.uint8)[i + 1:i + 1 - c])
            i += 1 - c
        else:
            out.append(np.full(c + 1, bytes(b)[i + 1], dtype=np.uint8))
            i += 2
    return np.concatenate(out).tobytes() if out else b""


def test_rle_decode_matches_restatement():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 127, 128, 129, 255, 1000, 5000):
        raw = rng.integers(0, 4, n, dtype=np.uint8)
        raw[: n // 3] = 9
        enc = X.rle_compress(raw.tobytes())
        want = _rle_numpy(enc)
        assert want == raw.tobytes()
        assert _rle(enc, n) == (n, want)
        assert E.rle_decode(enc, n) == want
    hand = bytes([2, 7, 256 - 3, 1, 2, 3, 127, 0, 0, 5])               # 3 x 7, literal 1 2 3, 128 x 0, 1 x 5
    want = bytes([7] * 3 + [1, 2, 3] + [0] * 128 + [5])
    assert _rle_numpy(hand) == want and _rle(hand, len(want)) == (len(want), want)
    assert _rle(b"", 4) == (0, b"")


def test_rle_decode_overrun_and_underrun():
    lib = pkg._lib.load()
    for data, cap, where in ((bytes([5, 1]), 5, b"output"),              # run of 6 into 5
                             (bytes([256 - 4, 1, 2, 3, 4]), 3, b"output"),  # literal of 4 into 3
                             (bytes([256 - 4, 1, 2, 3]), 10, b"input"),     # literal of 4, 3 bytes left
                             (bytes([1, 9, 3]), 10, b"input")):             # a count with no byte to repeat
        n, _ = _rle(data, cap)
        assert n == -1 and where in lib.shdr_last_error(), (data, lib.shdr_last_error())
        with pytest.raises(ValueError, match="overruns"):
            E.rle_decode(data, cap)
    assert _rle(bytes([3, 1]), 10) == (4, bytes([1] * 4))                  # underrun of the output: the caller checks the count


# --- read_payload on the writer's files ----------------------------------------------------------------------------
def _planes_of(payload):
    """the payload's chunks with the predictor / interleave undone (numpy restatement)"""
    out = []
    for c in range(len(payload.coded)):
        b = payload.data[payload.offsets[c]:payload.offsets[c + 1]].tobytes()
        out.append(X.unpredict(b) if payload.coded[c] else b)
    return out


@pytest.mark.parametrize("order", [X.INC, X.DEC])
@pytest.mark.parametrize("comp", [X.NONE, X.RLE, X.ZIPS, X.ZIP])
def test_read_payload_matches_writer(tmp_path, comp, order):
    h, w = 37, 13
    ch = {"R": (_image(h, w, 1), X.HALF), "G": (_image(h, w, 2), X.FLOAT), "B": (_image(h, w, 3), X.HALF),
          "A": (_image(h, w, 4), X.HALF), "Z": (np.arange(h * w, dtype=np.uint32).reshape(h, w), X.UINT)}
    rng = np.random.default_rng(5)
    for name, (img, _) in ch.items():                                          # rows that do not compress under ZIPS / RLE
        img[5:9] = rng.integers(0, 1 << 32, (4, w), dtype=np.uint64) if name == "Z" else rng.normal(0.0, 1e3, (4, w))
    path = str(tmp_path / "p.exr")
    info = X.write_exr(path, ch, comp, order, origin=(-7, -20))
    p = E.read_payload(path)
    hdr = p.header
    assert [c.name for c in hdr.channels] == ["A", "B", "G", "R", "Z"]
    assert [c.offset for c in hdr.channels] == [0, 2 * w, 4 * w, 8 * w, 10 * w] and hdr.row_bytes == info["row_bytes"] == 14 * w
    assert hdr.lines == X.LINES[comp] and hdr.n_chunks == len(info["chunks"]) and hdr.line_order == order
    assert hdr.data_window == (-7, -20, -7 + w - 1, -20 + h - 1)
    assert p.coded.tolist() == [int(c) for c in info["coded"]]
    if comp != X.NONE:
        assert p.coded.any() and (comp == X.ZIP or not p.coded.all())         # raw chunks occur too
    assert _planes_of(p) == info["chunks"]
    last = h - (hdr.n_chunks - 1) * hdr.lines
    assert p.offsets[-1] - p.offsets[-2] == last * hdr.row_bytes


def test_channel_list_order_is_sorted(tmp_path):
    path = str(tmp_path / "o.exr")
    ch = _rgb_channels(extra={"A": (_image(20, 9), X.FLOAT)})
    info = X.write_exr(path, ch, X.ZIP, list_order=["R", "G", "B", "A"])
    h = E.read_header(path)
    assert [c.name for c in h.channels] == ["A", "B", "G", "R"]
    assert _planes_of(E.read_payload(path)) == info["chunks"]


def test_file_list_includes_exr(tmp_path):
    for name in ("b.hdr", "a.exr", "c.exr", "d.txt", "e.hdr"):
        open(str(tmp_path / name), "wb").write(b"")
    assert D._posfix_list(str(tmp_path), None, "no_such_list") == ["a.exr", "b.hdr", "c.exr", "e.hdr"]
    only = tmp_path / "only"
    only.mkdir()
    open(str(only / "x.exr"), "wb").write(b"")
    assert D._posfix_list(str(only), None, "no_such_list") == ["x.exr"]
