"""The derivation behind the device scanline encoder, checked on the CPU: the host routine's greedy loop (csrc/api.cpp,
rle_component) equals "stretches -> runs capped at 127 -> tokens" (tests/hdr_rle_ref.py), run by run and in the per-position form
csrc/hdr_rle.hip computes.  Byte equality on every line family of the encoder tests; no GPU."""
import importlib

import numpy as np
import pytest

import hdr_rle_ref as R

pkg = importlib.import_module("singlehdr-tf2_amd")
IO = pkg.hdr_io

WIDTHS = (8, 9, 126, 127, 128, 129, 254, 255, 257, 300, 1000)


def _host_component(line):
    """the host routine's bytes for one component: a 1-row image whose other components are constant"""
    w = line.size
    img = np.zeros((1, w, 4), dtype=np.uint8)
    img[0, :, 0] = line
    data = IO.rle_encode(img)
    tail = len(R.encode_component(np.zeros(w, dtype=np.uint8))) * 3
    return data[4:len(data) - tail]


@pytest.mark.parametrize("w", WIDTHS)
def test_both_restatements_equal_the_host_loop_on_every_family(w):
    rng = np.random.default_rng(w)
    for name, line in R.families(w, rng).items():
        assert line.shape == (w,) and line.dtype == np.uint8, name
        want = _host_component(line)
        assert R.encode_component(line) == want, (w, name)
        assert R.encode_component_positions(line) == want, (w, name)


def test_known_scanlines():
    assert R.encode_component(np.full(8, 10, dtype=np.uint8)) == bytes([136, 10])
    assert R.encode_component(np.array([1, 1, 2, 2, 2, 2, 3, 3, 3], dtype=np.uint8)) == bytes([130, 1, 132, 2, 131, 3])
    assert R.encode_component(np.array([1, 1, 5, 2, 2, 2, 2, 3], dtype=np.uint8)) == bytes([3, 1, 1, 5, 132, 2, 1, 3])
    line = np.full(130, 7, dtype=np.uint8)                                  # 127 + 3: the rest of a long stretch is a gap of one run
    assert R.encode_component(line) == bytes([255, 7, 131, 7])
    line[-1] = 8                                                            # 127 + 2 + 1: two runs -> literals
    assert R.encode_component(line) == bytes([255, 7, 3, 7, 7, 8])


@pytest.mark.parametrize("seed", range(6))
def test_random_lines_dense_in_short_runs(seed):
    """random stretch lengths around every boundary of the rule (1..6, 126..130, 253..258) and random widths"""
    rng = np.random.default_rng(100 + seed)
    pool = np.array([1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 126, 127, 128, 129, 130, 253, 254, 255, 256, 257, 258, 381, 384])
    for _ in range(40):
        w = int(rng.integers(8, 1500))
        line = R._from_runs(w, rng.choice(pool, size=w).tolist(), first=int(rng.integers(0, 250)))
        want = _host_component(line)
        assert R.encode_component(line) == want
        assert R.encode_component_positions(line) == want


def test_whole_images_and_flat_widths():
    for h, w in ((3, 7), (2, 300), (1, 8), (1, 32768), (2, 32767)):
        img = R.family_image(h, w, seed=h + w)
        assert R.encode_image(img) == IO.rle_encode(img), (h, w)
    img = R.family_image(3, 257, seed=1)
    assert R.encode_image(img, R.encode_component_positions) == IO.rle_encode(img)
    assert np.array_equal(IO.rle_decode(R.encode_image(img), 3, 257), img)
