"""The scanline streams the Radiance readers are tested on: cases() is a list of (name, W, H, bytes), built once.

Well-formed content is the encoder's output (the host routine shdr_rgbe_rle_encode, which tests/test_hdr_rle_ref.py holds to the NumPy
restatement) for the line families of tests/hdr_rle_ref.py; the rest is built packet by packet here.  Shapes are the smallest at which
each part of a reader can go wrong; the module docstrings of the tests say which.
"""
import functools
import importlib

import numpy as np

import hdr_rle_ref as R

WIDTHS = (1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 514)
HEIGHTS = (1, 2, 3, 65)
MUTATIONS = (0, 1, 2, 127, 128, 129, 255)


def _encode(img):
    return importlib.import_module("singlehdr-tf2_amd").hdr_io.rle_encode(img)


def marker(w):
    return bytes((2, 2, w >> 8, w & 255))


def run(n, v):
    assert 1 <= n <= 127
    return bytes((128 + n, v))


def lit(values):
    values = bytes(values)
    assert len(values) <= 128
    return bytes((len(values),)) + values


def coded_line(w, *components):
    """marker + the four components as given (each a byte string of packets)"""
    assert len(components) == 4
    return marker(w) + b"".join(components)


def _image(h, w, seed):
    if w < 7:
        return np.random.default_rng(seed).integers(0, 256, size=(h, w, 4)).astype(np.uint8)
    return R.family_image(h, w, seed)


def _noisy_smooth_constant(h, w, seed):
    """rows whose four components are noisy, smooth (long stretches), constant and noisy again, rotating from row to row"""
    rng = np.random.default_rng(seed)
    kinds = [lambda: rng.integers(0, 256, size=w), lambda: np.repeat(rng.integers(0, 256, size=w // 40 + 1), 40)[:w],
             lambda: np.full(w, int(rng.integers(0, 256))), lambda: rng.integers(0, 256, size=w)]
    img = np.empty((h, w, 4), dtype=np.uint8)
    for y in range(h):
        for c in range(4):
            img[y, :, c] = kinds[(y + c) % 4]()
    return img


def _all_families_files(w, seed):
    """every family line of width w, eight to a file of two rows"""
    lines = list(R.families(w, np.random.default_rng(seed)).values())
    while len(lines) % 8:
        lines.append(lines[len(lines) % 5])
    return [np.stack(lines[i:i + 8]).reshape(2, 4, w).transpose(0, 2, 1).copy() for i in range(0, len(lines), 8)]


def small_coded():
    """9 x 3, every line coded"""
    return 9, 3, _encode(_image(3, 9, seed=91))


def small_mixed():
    """8 x 3: a flat line, a coded line, a flat line"""
    w = 8
    flat0 = bytes(range(10, 10 + 4 * w))
    flat2 = bytes(range(100, 100 + 4 * w))
    mid = coded_line(w, run(8, 5), lit(range(8)), run(3, 1) + lit((9, 8, 7, 6, 5)), lit((1, 2)) + run(6, 200))
    return w, 3, flat0 + mid + flat2


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, w, h, data):
        out.append((name, int(w), int(h), bytes(data)))

    # --- widths and heights: the encoder's output ---------------------------------------------------------------------------
    for w in WIDTHS:
        for h in HEIGHTS:
            add("families_%dx%d" % (w, h), w, h, _encode(_image(h, w, seed=3 * w + h)))
        if w >= 8:
            add("noisy_smooth_constant_%d" % w, w, 5, _encode(_noisy_smooth_constant(5, w, seed=w)))
    for i, img in enumerate(_all_families_files(32767, seed=5)):
        add("families_32767_%d" % i, 32767, 2, _encode(img))
    add("flat_32768", 32768, 1, _encode(R.family_image(1, 32768, seed=6)))

    # --- hand-built lines ------------------------------------------------------------------------------------------------------
    w = 16
    plain = run(16, 7)
    add("zero_count_start", w, 1, coded_line(w, b"\0" + run(16, 1), plain, plain, plain))
    add("zero_count_middle", w, 1, coded_line(w, run(5, 1) + b"\0" + lit(range(11)), plain, plain, plain))
    add("zero_count_before_next_component", w, 1, coded_line(w, plain, b"\0" + plain, b"\0" + plain, b"\0" + plain))
    add("zero_counts_in_a_row", w, 2, coded_line(w, b"\0\0\0" + run(9, 3) + b"\0\0" + lit(range(7)), plain, b"\0" * 40 + plain, plain) * 2)
    add("zero_count_behind_last_line", w, 1, coded_line(w, plain, plain, plain, plain) + b"\0")
    add("zero_count_behind_first_line", w, 2, coded_line(w, plain, plain, plain, plain) + b"\0" + coded_line(w, plain, plain, plain, plain))
    add("zero_counts_longer_than_a_window", w, 2, coded_line(w, plain, b"\0" * 3000 + plain, plain, lit(range(16))) * 2)
    w = 130
    add("literal_128", w, 1, coded_line(w, lit(range(128)) + lit((1, 2)), lit((1, 2)) + lit(range(128)), run(127, 9) + run(3, 8),
                                        run(1, 4) + run(127, 5) + run(1, 6) + run(1, 7)))
    add("ends_on_run_and_on_literal", w, 2, coded_line(w, lit(range(100)) + run(30, 1), run(30, 1) + lit(range(100)),
                                                       run(127, 0) + lit((1, 2, 3)), lit((1, 2, 3)) + run(127, 255)) * 2)
    w = 9
    ones = b"".join(lit((v,)) for v in range(9))
    add("one_byte_literals", w, 2, coded_line(w, ones, ones, ones, ones) * 2)
    w = 300
    ones = b"".join(lit((v & 255,)) for v in range(300))
    add("one_byte_literals_300", w, 1, coded_line(w, ones, ones, ones, ones))

    # --- framing ---------------------------------------------------------------------------------------------------------------
    w = 9
    code = coded_line(w, run(9, 1), lit(range(9)), run(4, 2) + run(5, 3), lit((7,)) + run(8, 9))
    flat = bytes((50 + i) & 255 for i in range(4 * w))
    add("flat_before_between_after", w, 5, flat + code + flat + code + flat)
    add("flat_starting_0202_other_width", w, 3, code + bytes((2, 2, 0, 10)) + flat[4:] + code)
    add("flat_starting_0202_high_byte", w, 2, bytes((2, 2, 1, 9)) + flat[4:] + code)
    for at in (1, 5, 32 - 4):                                        # the marker inside a flat line: a parse from it fails or leaves the file
        body = bytearray(flat)
        body[at:at + 4] = marker(w)
        add("flat_with_marker_at_%d" % at, w, 3, code + bytes(body) + code)
    w = 8
    inner = coded_line(w, run(8, 1), run(8, 2), run(8, 3), run(8, 4))                 # 12 bytes: a whole line inside a flat one
    flat8 = bytes((70 + i) & 255 for i in range(32))
    for at in (1, 4, 20):
        body = bytearray(flat8)
        body[at:at + 12] = inner
        add("flat_with_whole_line_at_%d" % at, w, 3, bytes(body) + inner + bytes(body))
        add("flat_with_whole_line_at_%d_last" % at, w, 2, inner + bytes(body))
    w = 12
    add("marker_inside_literal", w, 2, coded_line(w, lit((1, 2, 3) + tuple(marker(w)) + (4, 5, 6, 7, 8)), run(12, 0),
                                                  lit(tuple(marker(w)) * 3), run(12, 2)) * 2)
    w, h, data = small_coded()
    add("trailing_garbage", w, h, data + bytes(range(37)))
    add("trailing_marker", w, h, data + marker(w))
    add("trailing_cut_marker", w, h, data + marker(w)[:3])
    add("trailing_whole_line", w, h, data + data[:len(data) // 1])
    add("trailing_line_with_corrupt_run", w, h, data + marker(w) + run(10, 1))
    add("one_line_of_three", w, 1, data)
    # the dense case: W = 514 = 0x0202, the value 2 everywhere: every offset holds the marker (and the host routine, which reads the
    # first line as coded, refuses the file)
    add("dense_514", 514, 4, bytes((2,)) * (4 * 514 * 4))
    # the same where the host routine accepts the file: every flat line starts with a 3, so no line start is a marker
    dense_line = bytes((3,)) + bytes((2,)) * (4 * 514 - 1)
    add("dense_514_flat", 514, 4, dense_line * 4)
    add("dense_514_then_coded", 514, 3, dense_line * 2 + _encode(_image(1, 514, seed=8)))
    # 2 H + 64 line markers are decoded on the device, one more is left to the host routine: H = 1 and H = 3
    w = 8
    for h in (1, 3):
        body = inner * h
        cap = 2 * h + 64
        for extra, tag in ((cap - h, "at_cap"), (cap - h + 1, "over_cap"), (cap - h - 1, "under_cap")):
            add("markers_%s_h%d" % (tag, h), w, h, body + (marker(w) + b"\x77") * extra)
    flat_marked = bytearray(flat8)
    flat_marked[8:12] = marker(w)
    add("markers_at_cap_in_flat_lines", w, 66, bytes(flat_marked) * 66)                # 66 flat lines, 66 markers <= 2 * 66 + 64
    add("markers_over_cap_in_flat_lines", w, 1, bytes(flat_marked[:8]) + marker(w) * 6 + (marker(w) + b"\0") * 61)

    # --- refusals --------------------------------------------------------------------------------------------------------------
    for tag, (w, h, data) in (("coded", small_coded()), ("mixed", small_mixed())):
        for n in range(len(data)):
            add("prefix_%s_%d" % (tag, n), w, h, data[:n])
    w, h, data = small_coded()
    for at in range(len(data)):
        for v in MUTATIONS:
            if data[at] != v:
                body = bytearray(data)
                body[at] = v
                add("byte_%d_set_to_%d" % (at, v), w, h, body)
    add("size_0", 9, 1, b"")
    add("size_0_flat", 3, 2, b"")
    w = 16
    plain = run(16, 7)
    add("run_overshoots_by_one", w, 2, coded_line(w, plain, plain, plain, plain) + coded_line(w, plain, run(10, 1) + run(7, 2), plain, plain))
    add("literal_overshoots_by_one", w, 1, coded_line(w, plain, plain, run(10, 1) + lit(range(7)) + plain, plain))
    add("count_byte_is_last_run", w, 1, coded_line(w, plain, plain, plain, run(10, 1))[:-1])
    add("count_byte_is_last_literal", w, 1, coded_line(w, plain, plain, plain, run(10, 1) + bytes((6,))))
    add("data_ends_before_count_byte", w, 1, coded_line(w, plain, plain, plain, run(10, 1)))
    add("flat_line_one_byte_short", 7, 3, bytes(range(4 * 7 * 3 - 1)))
    return out


def by_name():
    return {c[0]: c for c in cases()}
