"""tests/imageio_ref.py on the CPU: the references against numpy where numpy has the operation, the preconditions of the exact cases,
the fp32 restatement (oracle/imageio.py) inside the per-element tolerance, and the WRONG MODELS -- the reference with one plausible
error each.  At the very inputs of tests/test_gpu_imageio_elem.py every wrong model must differ from the true reference in at least
one element by more than the family's tolerance (any bit for the exact families): a kernel with that error would fail there."""
import numpy as np
import pytest

import imageio_ref as R
from oracle import imageio as O

CUBIC_WRONG = {
    "reflected border": dict(border="reflect"),
    "taps s .. s+3": dict(first=0),
    "A = -0.5": dict(A=-0.5),
    "H and W scales swapped": dict(swap_scales=True),
    "align-corners coordinate": dict(coord="align_corners"),
}
PAD_WRONG = {
    "reflect without repeating the edge": lambda x, p: R.pad_symmetric(x, p, repeat_edge=False),
    "H/W pad swapped": lambda x, p: R.pad_symmetric(x, p, pad_hw=(min(p + 1, x.shape[1]), max(p - 1, 0))),
}
FLIP_WRONG = {
    "flip after the rotation": dict(order="rot_first"),
    "clockwise rotation": dict(clockwise=True),
    "k not reduced mod 4": dict(reduce_k=False),
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_references_agree_with_numpy():
    rng = np.random.default_rng(0)
    x = rng.random((2, 9, 7, 3)).astype(np.float32)
    for pad in (0, 1, 5, 7):
        assert np.array_equal(R.pad_symmetric(x, pad), np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)), "symmetric"))
    sq = rng.random((18, 7, 7, 3)).astype(np.float32)
    flip, k = np.array([f for f, _ in R.FLIP_ROT]), np.array([k for _, k in R.FLIP_ROT])
    got = R.flip_rot90(sq, flip, k, 255.0)
    for i in range(18):
        want = np.rot90(sq[i][:, ::-1] if flip[i] else sq[i], int(k[i]), axes=(0, 1)) / np.float32(255)
        assert np.array_equal(got[i], want), i
    # the identity resize returns the input; a constant image stays constant (the weights sum to one)
    y, S, T = R.cubic(x, (9, 7))
    assert np.array_equal(y, x.astype(np.float64)) and np.array_equal(S, np.abs(y)) and np.all(T >= S)
    y, _, _ = R.cubic(np.full((1, 5, 6, 1), 3.0), (11, 4))
    assert np.abs(y - 3.0).max() <= 1e-14


def test_cubic_coordinate_is_opencvs():
    """(float)((d + 0.5) * scale - 0.5), scale = 1 / (n_out / n_in) in double: spot values worked by hand"""
    idx, w = R.cubic_axis(4, 8)                   # scale 0.5: f = -0.25, 0.25, 0.75, ...
    assert idx[0].tolist() == [0, 0, 0, 1] and idx[1].tolist() == [0, 0, 1, 2] and idx[7].tolist() == [2, 3, 3, 3]
    t = 0.75
    want = [((-0.75 * (t + 1) + 3.75) * (t + 1) - 6) * (t + 1) + 3, (1.25 * t - 2.25) * t * t + 1]
    assert np.allclose(w[0, :2], want, rtol=0, atol=1e-15) and np.allclose(w.sum(axis=1), 1, rtol=0, atol=1e-15)
    # the fp32 rule of the parent commit drifts along a wide row; OpenCV's does not
    _, w_cv = R.cubic_axis(4000, 4032)
    _, w_32 = R.cubic_axis(4000, 4032, coord="fp32")
    assert np.abs(w_cv - w_32).max() > 1e-4


@pytest.mark.parametrize("case", R.CUBIC_EXACT, ids=R.case_id)
def test_cubic_exact_cases_are_exact(case):
    """the precondition of the bit-for-bit GPU test: at these inputs the fp32 restatement equals the float64 reference in bits"""
    _, _, ho, wo, _ = case
    for n in (1, 2):
        for c in (1, 3, 4):
            x = R.cubic_exact_input(case, n, c)
            y, _, _ = R.cubic(x, (ho, wo))
            assert np.array_equal(y.astype(np.float32).astype(np.float64), y), "reference not representable in fp32"
            assert np.array_equal(bits(O.resize_cubic(x, (ho, wo))), bits(y))


def test_cubic_exact_cases_catch_every_wrong_model():
    """any differing bit counts.  (No single case catches all: the identity resize only sees the tap shift.)"""
    for name, kw in CUBIC_WRONG.items():
        hits = 0
        for case in R.CUBIC_EXACT:
            x = R.cubic_exact_input(case, 2, 3)
            hits += not np.array_equal(bits(R.cubic(x, case[2:4], **kw)[0]), bits(R.cubic(x, case[2:4])[0]))
        assert hits >= 3, (name, hits)


def test_4x_case_is_exact_only_for_unit_inputs():
    """why (7, 5, 28, 20) runs with inputs in {-1, 0, 1}: with [-4, 4] the fp32 sums round"""
    x = np.random.default_rng(1).integers(-4, 5, size=(1, 7, 5, 3)).astype(np.float32)
    y, _, _ = R.cubic(x, (28, 20))
    assert not np.array_equal(bits(O.resize_cubic(x, (28, 20))), bits(y))


def test_fp32_weight_polynomial_within_its_derived_error():
    """the per-weight bounds E of the tolerance's derivation (test_gpu_imageio_elem.py), at 2^20 fractions t"""
    t = np.unique(np.concatenate([np.random.default_rng(2).random(1 << 20).astype(np.float32),
                                  np.float32([0, 0.5, np.nextafter(np.float32(1), np.float32(0)), 2.0 ** -24, 2.0 ** -12])]))
    f, A, one = np.float32, np.float32(-0.75), np.float32(1)
    c0 = ((A * (t + one) - f(5) * A) * (t + one) + f(8) * A) * (t + one) - f(4) * A
    c1 = ((A + f(2)) * t - (A + f(3))) * t * t + one
    c2 = ((A + f(2)) * (one - t) - (A + f(3))) * (one - t) * (one - t) + one
    c3 = one - c0 - c1 - c2
    t64 = t.astype(np.float64)
    w0 = ((-0.75 * (t64 + 1) + 3.75) * (t64 + 1) - 6) * (t64 + 1) + 3
    w1 = (1.25 * t64 - 2.25) * t64 * t64 + 1
    w2 = (1.25 * (1 - t64) - 2.25) * (1 - t64) * (1 - t64) + 1
    w3 = 1 - w0 - w1 - w2
    for got, want, bound in ((c0, w0, 27), (c1, w1, 5), (c2, w2, 5.7), (c3, w3, 39.8)):
        assert np.abs(got.astype(np.float64) - want).max() <= bound * R.U
    assert 2 * 39.8 <= R.B_TOL


@pytest.mark.parametrize("case", R.CUBIC_GENERAL, ids=R.case_id)
def test_cubic_general_cases(case):
    """the fp32 restatement alone stays within the per-element tolerance; at the wide rows the parent commit's coordinate leaves it"""
    n, h, w, c, ho, wo = case
    x = R.cubic_general_input(case)
    y, S, T = R.cubic(x, (ho, wo))
    tol = R.cubic_tol(S, T)
    err = np.abs(O.resize_cubic(x, (ho, wo)).astype(np.float64) - y)
    assert np.all(err <= tol), "fp32 restatement: worst err / tol = %.3g" % float((err / np.maximum(tol, 1e-300)).max())
    if case in R.CUBIC_WIDE:                      # the rule of the parent commit, where width makes the coordinate go wrong
        bad, _, _ = R.cubic(x, (ho, wo), coord="fp32")
        over = np.abs(bad - y) / tol              # worst element: 7 times the tolerance at 1408 -> 1400, 14 times at 4000 -> 4032
        assert over.max() > 5, over.max()


def test_cubic_general_cases_catch_every_wrong_model():
    """beyond the tolerance in at least one element.  (A source axis of one pixel ignores its coordinate, and a down-scaling never
    reaches index -2, where the two border rules part: no single case catches all; the first two catch every model.)"""
    for name, kw in CUBIC_WRONG.items():
        hits = []
        for case in R.CUBIC_GENERAL[:5]:
            x = R.cubic_general_input(case)
            y, S, T = R.cubic(x, case[4:])
            hits.append(bool(np.any(np.abs(R.cubic(x, case[4:], **kw)[0] - y) > R.cubic_tol(S, T))))
        assert all(hits[:2]), (name, hits)


@pytest.mark.parametrize("case", R.PAD_CASES, ids=R.case_id)
def test_pad_cases(case):
    x = R.pad_input(case)
    pad = case[4]
    want = R.pad_symmetric(x, pad)
    assert np.array_equal(want, np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)), "symmetric"))
    if pad == 0:
        return
    n, h, w, c, _ = case
    bad = PAD_WRONG["reflect without repeating the edge"](x, pad)
    assert h * w == 1 or not np.array_equal(bad, want)
    bad = PAD_WRONG["H/W pad swapped"](x, pad)
    assert bad.shape != want.shape or not np.array_equal(bad, want)


@pytest.mark.parametrize("case", R.FLIP_CASES, ids=R.case_id)
def test_flip_rot90_cases(case):
    s, c, d = case
    x, flip, k = R.flip_input(case)
    want = R.flip_rot90(x, flip, k, d)
    for i in range(len(k)):
        ref = np.rot90(x[i][:, ::-1] if flip[i] else x[i], int(k[i]), axes=(0, 1)) / np.float32(d)
        assert np.array_equal(want[i], ref), i
    if s == 1:
        return                                    # one pixel: every permutation is the identity
    for name, kw in FLIP_WRONG.items():
        assert not np.array_equal(R.flip_rot90(x, flip, k, d, **kw), want), name


def test_rgbe_special_pixels_mean_what_they_say():
    px, expect = R.rgbe_pixels()
    got = O.rgbe_encode(px)
    assert got[1].tolist() == [128, 64, 32, 129]
    for row, ch, byte in expect:                  # the truncating cast gives j at j 2^(e-8) and j - 1 one fp32 step below
        assert got[row, ch] == byte, (row, ch, byte, px[row])
    t = np.float32(1e-32)
    zero = [r for r in range(len(px)) if px[r].max() < 1e-32]
    assert len(zero) >= 4 and not got[zero].any()
    assert got[np.flatnonzero((px == t).any(axis=1) & (px.max(axis=1) == t))].any() == (float(t) >= 1e-32)
    assert len(R.rgbe_input(1)) == 1 and len(R.rgbe_input(R.LAUNCH_THREADS + 3)) == R.LAUNCH_THREADS + 3


def test_large_cases_take_a_second_grid_stride_trip():
    n, h, w, c, ho, wo = R.CUBIC_GENERAL[-1]
    assert n * ho * wo * c > R.LAUNCH_THREADS
    n, h, w, c, pad = R.PAD_CASES[-1]
    assert n * (h + 2 * pad) * (w + 2 * pad) * c > R.LAUNCH_THREADS
    s, c, _ = R.FLIP_CASES[-1]
    assert len(R.FLIP_ROT) * s * s * c > R.LAUNCH_THREADS
    for ch in range(3):
        assert len(np.unique(R.u8_pixels(256)[:, ch])) == 256
