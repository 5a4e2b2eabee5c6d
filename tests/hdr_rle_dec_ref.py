"""An independent reader of Radiance scanline data, written from the format and not from csrc/hdr_rle_dec.h: the oracle of the host
twin shdr_rgbe_rle_decode_status and, through it, of the device decoder.

The format: the lines of an H x W picture follow one another without an index.  When 8 <= W <= 32767 and a line starts with the four
bytes 02 02 W>>8 W&255 it is run-length coded: the R, G, B and E bytes of the line in turn, each as packets until W bytes are there.
A packet is a count byte n and, for n > 128, one byte to be repeated n - 128 times, else n bytes as they are.  Any other line is W
pixels of four bytes.  A reader must refuse a packet that does not fit the line or the data.

decode() returns (pixels, consumed) or (status, line, stop): the status codes are SHDR_RGBE_DEC_* of include/shdr.h, `line` is the
scanline that could not be read and `stop` the offset the reader stood at: the count byte of the offending packet, the end of the data
when a count byte is missing, or the first byte of a flat line that is not all there.
"""
import numpy as np

OK, TRUNCATED, CORRUPT_RUN, CORRUPT_LITERAL, TRUNCATED_FLAT, FALLBACK = range(6)


class Refused(Exception):
    def __init__(self, status, stop):
        Exception.__init__(self, status, stop)
        self.status, self.stop = status, stop


def _component(buf, at, width):
    """(bytes of one component, offset behind its last packet)"""
    got = []
    have = 0
    while have < width:
        if at >= len(buf):
            raise Refused(TRUNCATED, at)
        n = buf[at]
        if n > 128:
            if at + 1 >= len(buf):
                raise Refused(TRUNCATED, at)
            if have + n - 128 > width:
                raise Refused(CORRUPT_RUN, at)
            got.append(np.full(n - 128, buf[at + 1], dtype=np.uint8))
            have += n - 128
            at += 2
        else:
            if at + 1 + n > len(buf):
                raise Refused(TRUNCATED, at)
            if have + n > width:
                raise Refused(CORRUPT_LITERAL, at)
            got.append(np.frombuffer(buf[at + 1:at + 1 + n], dtype=np.uint8))
            have += n
            at += 1 + n
    return np.concatenate(got), at


def decode(data, width, height):
    """bytes -> (uint8 [height, width, 4], consumed) or (status, line, stop)"""
    buf = bytes(data)
    marker = bytes((2, 2, (width >> 8) & 255, width & 255)) if 8 <= width <= 32767 else None
    img = np.zeros((height, width, 4), dtype=np.uint8)
    at = 0
    for y in range(height):
        if marker is not None and buf[at:at + 4] == marker:
            at += 4
            for c in range(4):
                try:
                    img[y, :, c], at = _component(buf, at, width)
                except Refused as r:
                    return r.status, y, r.stop
        else:
            if len(buf) - at < 4 * width:
                return TRUNCATED_FLAT, y, at
            img[y] = np.frombuffer(buf[at:at + 4 * width], dtype=np.uint8).reshape(width, 4)
            at += 4 * width
    return img, at


def count_candidates(data, width):
    """offsets that hold the line marker of this width: what the device decoder counts against its cap of 2 H + 64"""
    if not 8 <= width <= 32767:
        return 0
    buf, marker = bytes(data), bytes((2, 2, width >> 8, width & 255))
    n, at = 0, buf.find(marker)
    while at >= 0:
        n += 1
        at = buf.find(marker, at + 1)
    return n


MESSAGES = {
    TRUNCATED: "rgbe_rle_decode: truncated data in scanline %d",
    CORRUPT_RUN: "rgbe_rle_decode: corrupt run in scanline %d",
    CORRUPT_LITERAL: "rgbe_rle_decode: corrupt literal in scanline %d",
    TRUNCATED_FLAT: "rgbe_rle_decode: truncated data in flat scanline %d",
}
