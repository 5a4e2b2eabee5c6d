"""The validation-metric kernels (csrc/metrics.hip: pair_moments, pair_moments_final, hdr_metrics, hdr_metrics_final, tonemap_u8)
through the C ABI, on inputs whose answer has no rounding excuse, at the shapes where the tile fold, the block cap and the alignment
paths change.

Exact inputs (metrics_ref.exact_pair): gt holds multiples of 2^-10 in [2^-4, 1] with an exact 1.0 per image, pred = gt + delta with
delta in +-{2^-4, 2^-6} chosen by the OWNERSHIP CLASS of the pixel in the kernel's tiling.  Without normalisation the scales are 1 and
the peak is 1, p - g = delta and delta^2 are exact in float32, the float64 sums are exact in any order, and mse_l must EQUAL
sum(delta^2) / cnt bit for bit: a pixel counted twice or not at all, a dropped tile partial or a mis-indexed image changes the sum.
With normalisation the float64 sums of the images are exact too, so both scales and the peak must equal the reference bit for bit.

Shapes (TH x TW = 16 x 32 windows per tile, asserted):
    (11, 11)    one window
    (27, 43)    2 x 2 tiles, the second of one window
    (49, 83)    3 x 3 tiles: an interior tile and partial last tiles
    (267, 522)  17 x 16 = 272 tiles (the final kernel's second trip of 256), 418 122 values: no multiple of 4 -> the scalar loads;
                the moments grid is capped at 64 blocks (103 wanted)
    (268, 522)  272 tiles, 419 688 values: float4 loads, 7 grid-stride trips of 64 x 256 float4

Every call goes through shdr._lib with each output and a workspace of EXACTLY shdr_metrics_workspace_bytes between guard words; after
each case the _ops wrapper must return the same bits."""
import ctypes
import functools
import re
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import ROOT, quantised_image
from test_gpu_conv_x3_exact import E_ALIGN, E_NULL, E_SHAPE
from test_gpu_metrics import LAWS, check, inputs, reference
from test_gpu_tape_f32 import LOGF
from test_gpu_wgrad_f32_exact import P, guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

TH, TW = 16, 32
SHAPES = [(11, 11), (27, 43), (49, 83), (267, 522), (268, 522)]
LARGE = SHAPES[3:]
KEYS = ("mse_l", "mse_mu", "l1_logc", "ssim_mu", "peak", "scale_pred", "scale_gt")
U = 2.0 ** -24
POWF = 8                                    # powf: 4 ulps (ASSUMED: no accuracy table of the device library is at hand)
LOG1PF = LOGF                               # log1pf: taken as logf, 2 ulps (assumed, test_gpu_tape_f32.py)


@pytest.fixture(scope="module")
def K(shdr):
    assert shdr._ops.METRICS_TILE == (TH, TW)
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def bits(t):
    return t.contiguous().view(torch.int64)


def workspace(lib, n, h, w):
    nbytes = lib.shdr_metrics_workspace_bytes(n, h, w)
    tiles = -(-(h - 10) // TH) * -(-(w - 10) // TW)
    blocks = min(max(-(-h * w * 3 // 4096), 1), 64)
    assert nbytes == n * max(tiles, blocks) * 32, (nbytes, tiles, blocks)
    return guarded(nbytes // 8, torch.float64)


def run_abi(lib, pred, gt, normalise, what, mu=5000.0):
    """both ABI calls on device tensors [N, H, W, 3] (any 4-byte aligned views); every output and the exactly sized workspace sit
    between guards.  Returns the seven outputs, float64 [N]."""
    n, h, w, _ = pred.shape
    wsb, ws = workspace(lib, n, h, w)
    out = {k: guarded(n, torch.float64) for k in KEYS}
    v = {k: out[k][1] for k in KEYS}
    rc = lib.shdr_pair_moments_f32(P(pred), P(gt), n, h, w, int(normalise), P(v["scale_pred"]), P(v["scale_gt"]), P(v["peak"]), P(ws),
                                   stream())
    assert rc == 0, (what, lib.shdr_last_error())
    rc = lib.shdr_hdr_metrics_f32(P(pred), P(gt), n, h, w, mu, P(v["scale_pred"]), P(v["scale_gt"]), P(v["peak"]), P(v["mse_l"]),
                                  P(v["mse_mu"]), P(v["l1_logc"]), P(v["ssim_mu"]), P(ws), stream())
    assert rc == 0, (what, lib.shdr_last_error())
    guards_intact(wsb, ws.numel(), what + " workspace")
    for k in KEYS:
        guards_intact(out[k][0], n, what + " " + k)
    return {k: v[k].clone() for k in KEYS}


def run_moments(lib, pred, gt, normalise, what):
    n, h, w, _ = pred.shape
    wsb, ws = workspace(lib, n, h, w)
    out = [guarded(n, torch.float64) for _ in range(3)]
    rc = lib.shdr_pair_moments_f32(P(pred), P(gt), n, h, w, int(normalise), P(out[0][1]), P(out[1][1]), P(out[2][1]), P(ws), stream())
    assert rc == 0, (what, lib.shdr_last_error())
    guards_intact(wsb, ws.numel(), what + " workspace")
    for b, _ in out:
        guards_intact(b, n, what)
    return [v.clone() for _, v in out]                      # scale_pred, scale_gt, peak


def wrapper_agrees(K, got, pred, gt, normalise, what):
    again = K.hdr_metrics(pred, gt, normalise=normalise)
    for k in KEYS:
        assert torch.equal(bits(again[k]), bits(got[k])), (what, k, again[k], got[k])


def host(got):
    return {k: v.cpu().numpy() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def exact(hw, n=3):
    pred, gt, delta = R.exact_pair((n,) + hw, TH, TW, seed=100 * hw[0] + hw[1])
    for a in (pred, gt, delta):
        a.setflags(write=False)
    return pred, gt, delta


@functools.lru_cache(maxsize=None)
def exact_reference(hw, normalise):
    pred, gt, _ = exact(hw)
    return R.hdr_metrics(pred, gt, normalise)


def offset_view(a, off):
    """the values of `a` in a device view that starts `off` floats past a 16-byte boundary, inside a larger guarded buffer"""
    buf, view = guarded(a.size + 4, torch.float32)
    t = view[off:off + a.size]
    assert t.data_ptr() % 16 == 4 * off
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return buf, t.view(a.shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# A1  exact inputs, normalise = False
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_mse_l_is_exact_by_ownership_class(K, lib, hw):
    """gap 1 (272 tiles: the `t += 256` trip of hdr_metrics_final_kernel) and the seam ownership of hdr_metrics_kernel: mse_l equals
    sum(delta^2) / cnt / peak^2 bit for bit; the other outputs meet the bars of test_gpu_metrics.py"""
    pred, gt, delta = exact(hw)
    ref = exact_reference(hw, False)
    cnt = float(hw[0]) * float(hw[1]) * 3.0
    want = (delta.astype(np.float64) ** 2).sum(axis=(1, 2, 3)) / cnt / (1.0 * 1.0)
    assert np.array_equal(want, ref["mse_l"]) and len(set(want)) == 3                  # the reference's own sum is exact too
    p, g = dev(pred), dev(gt)
    got = run_abi(lib, p, g, False, "exact %s" % (hw,))
    h = host(got)
    assert np.array_equal(h["mse_l"], want), (h["mse_l"], want, (h["mse_l"] - want) * cnt)
    assert np.array_equal(h["peak"], np.ones(3)) and np.array_equal(h["scale_pred"], np.ones(3))
    check(got, ref, "exact %s" % (hw,))
    wrapper_agrees(K, got, p, g, False, "exact %s" % (hw,))


PROBE_ROWS = [0, 15, 16, 31, 32, 38, 39, 48]
PROBE_COLS = [0, 31, 32, 63, 64, 72, 73, 82]


def test_single_pixel_is_counted_once_wherever_it_lies(K, lib):
    """gap 1, seams: one image per probed pixel of 49 x 83 (tile origins, last owned and first foreign lines, both sides of the last
    window 38 | 39 and 72 | 73, the image corners); pred differs from gt in ONE value by 2^-3, so mse_l = 2^-6 / cnt exactly for
    every image -- nothing dilutes a seam"""
    hgt, wid = 49, 83
    rng = np.random.default_rng(4983)
    n = len(PROBE_ROWS) * len(PROBE_COLS)
    gt = rng.integers(64, 1025, size=(n, hgt, wid, 3)).astype(np.float64) / 1024.0
    gt[:, 5, 5, 0] = 1.0
    pred = gt.copy()
    i = 0
    for y in PROBE_ROWS:
        for x in PROBE_COLS:
            pred[i, y, x, i % 3] += 0.125
            i += 1
    p, g = dev(pred), dev(gt)
    got = run_abi(lib, p, g, False, "single pixel")
    want = np.full(n, 2.0 ** -6 / (hgt * wid * 3.0))
    m = got["mse_l"].cpu().numpy()
    bad = np.flatnonzero(m != want)
    assert bad.size == 0, [(PROBE_ROWS[b // 8], PROBE_COLS[b % 8], m[b] / want[b]) for b in bad]
    wrapper_agrees(K, got, p, g, False, "single pixel")


def test_negative_pred_takes_the_clamp(K, lib):
    """negative elements of pred give p = 0 and d = -g, exact: g^2 is a multiple of 2^-20 below 2^0"""
    hw = (49, 83)
    pred, gt, _ = exact(hw)
    pred = pred.copy()
    rng = np.random.default_rng(7)
    neg = rng.random(pred.shape) < 0.2
    pred[neg] = -pred[neg] - np.float32(0.5)
    ref = R.hdr_metrics(pred, gt, False)
    p64, g64 = np.maximum(pred.astype(np.float64), 0.0), gt.astype(np.float64)
    want = ((p64 - g64) ** 2).sum(axis=(1, 2, 3)) / (49 * 83 * 3.0)
    assert np.array_equal(want, ref["mse_l"])
    p, g = dev(pred), dev(gt)
    got = run_abi(lib, p, g, False, "negative pred")
    assert np.array_equal(got["mse_l"].cpu().numpy(), want)
    check(got, ref, "negative pred")
    wrapper_agrees(K, got, p, g, False, "negative pred")


# SSIM of a plane against itself.  With a == b bit for bit the staged planes, the shifts and the five moments come out in equal
# pairs (the same operations on the same values), so va = vb = cab = v and mua = mub = m, and one window's term is
#     ((2 m m + C1) (2 v + C2)) / ((m m + m m + C1) (v + v + C2)).
# 2 v and v + v are exact and equal, so the second factors are the same float X.  The first factors A = rd(2 rd(m m) + C1) and
# B = rd(rd(m m + m m) + C1) -- or their fused forms, metrics.hip is built with contraction allowed -- each carry at most one rounding
# of the size of 2 m m and one of the sum: they differ by at most 3 units of 2^-24.  rd(A X), rd(B X) and the division add one each:
# 6 per window.  A thread adds up to four windows in float32 (3 roundings of a sum the size of the total), the rest is float64: k = 9.
K_SSIM_SELF = 9


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: "%dx%d" % s)
def test_identical_images_count_the_windows(K, lib, hw, normalise):
    """gap 1 again, through ssim_mu: pred bit-equal to gt gives three exact zeros and |ssim_mu - 1| <= 9 * 2^-24 = 5.4e-7, where ONE
    missing or doubled window of (268, 522) is 1 / (258 * 512) / 3 = 2.5e-6"""
    _, gt, _ = exact(hw)
    g = dev(gt)
    p = g.clone()
    got = run_abi(lib, p, g, normalise, "identical %s" % (hw,))
    h = host(got)
    for k in ("mse_l", "mse_mu", "l1_logc"):
        assert np.array_equal(h[k], np.zeros(3)) and not np.signbit(h[k]).any(), (k, h[k])
    worst = float(np.abs(h["ssim_mu"] - 1.0).max())
    print("identical %s normalise=%s: |ssim_mu - 1| = %.3g (bar %.3g)" % (hw, normalise, worst, K_SSIM_SELF * U))
    assert worst <= K_SSIM_SELF * U, h["ssim_mu"] - 1.0
    wrapper_agrees(K, got, p, g, normalise, "identical")


# ---------------------------------------------------------------------------------------------------------------------------------
# A2  moments
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(49, 83)] + LARGE, ids=lambda s: "%dx%d" % s)
def test_moments_are_exact_in_every_layout(K, lib, hw):
    """gap 2 (64-block cap: 103 blocks wanted at both large shapes, so every block makes grid-stride trips) and gap 3 (aligned bases
    with n_per % 4 == 0 take float4 loads; a pred or a gt that starts 4 bytes in takes the scalar loop): scale_pred, scale_gt and peak
    equal the reference bit for bit in all three layouts.  Image 0 keeps its maximum in its LAST element: a float4 loop run where it
    must not be drops the tail of (267, 522) and misses it."""
    pred, gt, _ = exact(hw)
    ref = exact_reference(hw, True)
    assert gt[0].reshape(-1)[-1] == 1.0
    n_per = hw[0] * hw[1] * 3
    assert (n_per % 4 == 0) == (hw == (268, 522)) and (-(-n_per // 4096) > 64) == (hw in LARGE)
    layouts = {"aligned": (0, 0), "pred + 4 bytes": (1, 0), "gt + 4 bytes": (0, 1)}
    for name, (op, og) in layouts.items():
        bp, p = offset_view(pred, op)
        bg, g = offset_view(gt, og)
        what = "moments %s %s" % (hw, name)
        sp, sg, pk = (t.cpu().numpy() for t in run_moments(lib, p, g, True, what))
        assert np.array_equal(sp, ref["scale_pred"]), (what, sp, ref["scale_pred"])
        assert np.array_equal(sg, ref["scale_gt"]), (what, sg, ref["scale_gt"])
        assert np.array_equal(pk, ref["peak"]), (what, pk, ref["peak"])
        assert len(set(sg)) == 3
        one = run_moments(lib, p, g, False, what + " raw")
        assert all(np.array_equal(t.cpu().numpy(), np.ones(3)) for t in one), what
        w = K.pair_moments(p, g, normalise=True)
        assert np.array_equal(torch.stack(w).cpu().numpy(), np.stack([sp, sg, pk])), what
        assert bool((bp[64 + op + pred.size:] == bp[0]).all()) and bool((bg[:64] == bg[0]).all())       # inputs are only read


def test_metrics_agree_across_layouts(K, lib):
    """gap 3 through the fused pass: the seven outputs of the offset views are the bits of the aligned call"""
    hw = (268, 522)
    pred, gt, _ = exact(hw)
    base = run_abi(lib, dev(pred), dev(gt), True, "aligned")
    for op, og in ((1, 0), (0, 1), (3, 2)):
        _, p = offset_view(pred, op)
        _, g = offset_view(gt, og)
        got = run_abi(lib, p, g, True, "offset %d %d" % (op, og))
        for k in KEYS:
            assert torch.equal(bits(got[k]), bits(base[k])), (op, og, k)
        wrapper_agrees(K, got, p, g, True, "offset")
    check(base, exact_reference(hw, True), "aligned, normalised")


def test_negative_mean_ground_truth(K, lib):
    """gap 5: a gt of negative mean and mixed signs has a negative scale, g = max(s_g gt, 0) keeps the NEGATIVE pixels and the peak is
    s_g * min(gt) (`fg >= 0 ? mx : mn`): peak and the scales' signs exact, everything at the bars of test_gpu_metrics.py"""
    rng = np.random.default_rng(55)
    shape = (3, 49, 83, 3)
    gt = -(quantised_image(rng, shape) * rng.uniform(1.0, 4.0, shape)) * np.array([1.0, 2.5, 0.4])[:, None, None, None]
    flip = rng.random(shape) < 0.25
    gt = np.where(flip, -0.5 * gt, gt).astype(np.float32)
    pred = (gt * (1.0 + 0.05 * rng.standard_normal(shape))).astype(np.float32)
    assert (gt.mean(axis=(1, 2, 3)) < 0).all() and (gt > 0).any() and (gt < 0).any()
    ref = R.hdr_metrics(pred, gt, True)
    assert (ref["scale_gt"] < 0).all() and (ref["peak"] > 0).all()
    assert np.array_equal(ref["peak"], ref["scale_gt"] * gt.min(axis=(1, 2, 3)).astype(np.float64))
    p, g = dev(pred), dev(gt)
    got = run_abi(lib, p, g, True, "negative mean")
    check(got, ref, "negative mean")
    wrapper_agrees(K, got, p, g, True, "negative mean")


def test_power_of_two_invariance(K, lib):
    """without normalisation, multiplying both images by 2^12 or 2^-12 scales p, g and the peak exactly: mse_l, mse_mu and ssim_mu
    keep their bits (l1_logc is not homogeneous)"""
    pred, gt = inputs((3, 2 * TH + 9, 2 * TW + 11), "quantised")
    base = run_abi(lib, dev(pred), dev(gt), False, "x1")
    for s in (2.0 ** 12, 2.0 ** -12):
        got = run_abi(lib, dev(pred * np.float32(s)), dev(gt * np.float32(s)), False, "x%g" % s)
        for k in ("mse_l", "mse_mu", "ssim_mu"):
            assert torch.equal(bits(got[k]), bits(base[k])), (s, k, got[k], base[k])
        assert torch.equal(got["peak"], base["peak"] * s)


# ---------------------------------------------------------------------------------------------------------------------------------
# A3  batch independence
# ---------------------------------------------------------------------------------------------------------------------------------
def five_images():
    rng = np.random.default_rng(31)
    shape = (5, 49, 83, 3)
    gt = quantised_image(rng, shape) * rng.uniform(1.0, 4.0, shape) * np.array([1.0, 2.5, 0.4, 1.7, 0.8])[:, None, None, None]
    pred = gt * (1.0 + 0.05 * rng.standard_normal(shape))
    return pred.astype(np.float32), gt.astype(np.float32)


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "normalised"])
def test_images_of_a_batch_do_not_see_each_other(K, lib, normalise):
    """gap 6: every output of image n of a batch of five is the bits of the call on that image alone; then image 1 gets gt = 0 and
    image 3 gets gt <= 0 with negative values -- both have peak 0 without normalisation, and the header's IEEE results: which output
    is NaN and which is inf is the reference's answer -- while images 0, 2 and 4 keep their solo bits"""
    pred, gt = five_images()
    solo = [run_abi(lib, dev(pred[i:i + 1]), dev(gt[i:i + 1]), normalise, "solo %d" % i) for i in range(5)]
    p, g = dev(pred), dev(gt)
    got = run_abi(lib, p, g, normalise, "batch")
    for i in range(5):
        for k in KEYS:
            assert torch.equal(bits(got[k][i:i + 1]), bits(solo[i][k])), (i, k)
    wrapper_agrees(K, got, p, g, normalise, "batch")

    gt = gt.copy()
    gt[1] = 0.0
    gt[3] = np.where(gt[3] > np.median(gt[3]), 0.0, -gt[3])
    assert (gt[3] <= 0).all() and (gt[3] < 0).any() and (gt[3] == 0).any() and (pred[1] > 0).any()
    with np.errstate(all="ignore"):
        ref = R.hdr_metrics(pred, gt, normalise)
    p, g = dev(pred), dev(gt)
    got = run_abi(lib, p, g, normalise, "batch with black images")
    h = host(got)
    for i in (0, 2, 4):
        for k in KEYS:
            assert torch.equal(bits(got[k][i:i + 1]), bits(solo[i][k])), (i, k)
    for i in (1, 3):
        for k in KEYS:
            a, b = h[k][i], ref[k][i]
            print("image %d %s: device %r, reference %r" % (i, k, a, b))
            if np.isnan(b):
                assert np.isnan(a), (i, k, a)
            elif np.isinf(b):
                assert a == b, (i, k, a, b)
            elif k == "peak":
                assert a == b, (i, k, a, b)
            elif k == "ssim_mu":
                assert abs(a - b) <= 1e-5, (i, k, a, b)
            else:
                assert abs(a - b) <= 1e-5 * abs(b), (i, k, a, b)
    assert ref["peak"][1] == 0.0 and np.isinf(ref["mse_l"][1]) and np.isnan(ref["mse_mu"][1]) and np.isnan(ref["ssim_mu"][1])
    assert np.isfinite(ref["l1_logc"][1])
    if not normalise:
        assert ref["peak"][3] == 0.0 and np.isinf(ref["mse_l"][3]) and np.isnan(ref["ssim_mu"][3])
    wrapper_agrees(K, got, p, g, normalise, "batch with black images")


# ---------------------------------------------------------------------------------------------------------------------------------
# A4  the random laws of test_gpu_metrics.py at the two large shapes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("hw", LARGE, ids=lambda s: "%dx%d" % s)
def test_random_laws_at_the_large_shapes(K, lib, hw, law, normalise):
    """gaps 1 and 2 on rounded data: 272 tiles and the capped moments grid, at the 1e-5 bars of test_gpu_metrics.py"""
    shape = (2,) + hw
    pred, gt = inputs(shape, law)
    p, g = dev(pred), dev(gt)
    got = run_abi(lib, p, g, normalise, "%s %s" % (hw, law))
    check(got, reference(shape, law, normalise), "%s %s normalise=%s" % (shape, law, normalise))
    wrapper_agrees(K, got, p, g, normalise, law)


# ---------------------------------------------------------------------------------------------------------------------------------
# A5  tonemap_u8
# ---------------------------------------------------------------------------------------------------------------------------------
def stream_grid_cap():
    src = open(os.path.join(ROOT, "singlehdr-tf2_amd", "csrc", "shdr_internal.h")).read()
    m = re.search(r"inline int stream_grid\(.*?if \(g > (\d+) \* (\d+)\)", src, re.S)
    return int(m.group(1)) * int(m.group(2))


# Units of 2^-24 relative to the value 255 T^(1/2.2), for T > 0 (T = 0 gives code 0 exactly):
#   v = s x                                   1     (exact when s = 1)
#   q = v / peak                              1     (the peaks used are float32 numbers)
#   mu q                                      1
#   log1pf                                    LOG1PF = 4; its argument's 3 units pass with a factor a / ((1 + a) log1p(a)) <= 1
#   inv_log (a rounded constant) and the product   2
#   => T to 3 + 4 + 2 = 9 units, through T^(1/2.2):  ceil(9 / 2.2) = 5
#   the exponent 1 / 2.2 rounded to float32: T^(e (1 + d)) = T^e exp(e d ln T), |ln T| <= 3 asserted below:  ceil(3 / 2.2) = 2
#   powf                                      POWF = 8 (ASSUMED)
#   255 * ...                                 1
K_TONEMAP = 5 + 2 + POWF + 1


@pytest.mark.parametrize("size", [(2, 12, 13), (2, 520, 520)], ids=lambda s: "%dx%dx%d" % s)
def test_tonemap_u8_codes(K, lib, size):
    """gap 4 (a non-NULL `scale`; every caller passes NULL) and the stream_grid cap (2 x 520 x 520 pixels > 2048 x 256): the codes EQUAL
    the float64 reference wherever the float64 value is further than value * 16 * 2^-24 from a rounding tie; nearer, they may differ
    by one.  At most 0.5 % of a case may be that near."""
    n, h, w = size
    assert (n * h * w > stream_grid_cap() * 256) == (size == (2, 520, 520))
    rng = np.random.default_rng(12 * h + w)
    x = (rng.integers(0, 1025, size=(n, h, w, 3)) / 1024.0 * rng.uniform(1.0, 4.0, (n, h, w, 3))).astype(np.float32)
    x[:, 3, 4] = 0.0
    x[:, 5, 6, 1] = -1.0
    scales = np.array([0.75, 1.5], dtype=np.float32)
    peaks = np.array([2.0, 3.5], dtype=np.float32)
    xd = dev(x)
    pk = torch.from_numpy(peaks.astype(np.float64)).cuda()
    sc = torch.from_numpy(scales.astype(np.float64)).cuda()
    for use_scale in (True, False):
        for rev in (0, 1):
            what = "tonemap %s scale=%s reverse=%d" % (size, use_scale, rev)
            assert x.size % 4 == 0
            buf, words = guarded(x.size // 4)                    # the codes, four to a guarded 32-bit word
            y = words.view(torch.uint8)
            rc = lib.shdr_tonemap_u8_f32(P(xd), P(sc) if use_scale else None, P(pk), P(y), n, h, w, 5000.0, rev, stream())
            assert rc == 0, (what, lib.shdr_last_error())
            guards_intact(buf, x.size // 4, what)
            got = y.view(n, h, w, 3).cpu().numpy()
            excluded, worst_excess = 0, 0.0
            for i in range(n):
                val, t = R.tonemap_value(x[i], float(peaks[i]), bool(rev), 5000.0, float(scales[i]) if use_scale else None)
                assert (t[t > 0] >= np.exp(-3.0)).all()
                code = np.rint(val)
                tie = np.abs(val - (np.floor(val) + 0.5))
                near = tie <= val * K_TONEMAP * U
                diff = got[i].astype(np.int64) - code.astype(np.int64)
                assert (diff[~near] == 0).all(), (what, i, int((diff[~near] != 0).sum()))
                assert (np.abs(diff) <= 1).all(), what
                wrong = diff != 0                  # a differing code bounds the device's error from below: the distance to the tie
                if wrong.any():
                    worst_excess = max(worst_excess, float((tie[wrong] / (val[wrong] * U)).max()))
                excluded += int(near.sum())
                assert (got[i][t == 0] == 0).all() and (got[i][t == 1] == 255).all() and (t == 0).sum() >= 4 and (t == 1).any()
            print("%s: %.3f %% within %d units of a tie; worst observed distance of a differing code %.2f units"
                  % (what, 100.0 * excluded / x.size, K_TONEMAP, worst_excess))
            assert excluded <= 0.005 * x.size, (what, excluded)
            if not use_scale:
                again = K.tonemap_u8(xd, peak=pk, reverse_channels=bool(rev))
                assert torch.equal(again.reshape(-1), y), what


# ---------------------------------------------------------------------------------------------------------------------------------
# A6  refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(lib):
    n, h, w = 2, 27, 43
    x = torch.rand(n, h, w, 3, device="cuda")
    wsb, ws = workspace(lib, n, h, w)
    out = [guarded(n, torch.float64) for _ in range(7)]
    o = [P(v) for _, v in out]
    st = stream()
    for nn, hh, ww in ((n, 10, w), (n, h, 10), (0, h, w), (-1, h, w)):
        assert lib.shdr_pair_moments_f32(P(x), P(x), nn, hh, ww, 1, o[0], o[1], o[2], P(ws), st) == E_SHAPE
        assert lib.shdr_hdr_metrics_f32(P(x), P(x), nn, hh, ww, 5000.0, o[0], o[1], o[2], o[3], o[4], o[5], o[6], P(ws), st) == E_SHAPE
    assert lib.shdr_pair_moments_f32(P(x), P(x), 65536, h, w, 1, o[0], o[1], o[2], P(ws), st) == E_SHAPE
    assert lib.shdr_hdr_metrics_f32(P(x), P(x), n, h, w, 0.0, o[0], o[1], o[2], o[3], o[4], o[5], o[6], P(ws), st) == E_SHAPE
    assert lib.shdr_pair_moments_f32(None, P(x), n, h, w, 1, o[0], o[1], o[2], P(ws), st) == E_NULL
    assert lib.shdr_pair_moments_f32(P(x), P(x), n, h, w, 1, o[0], None, o[2], P(ws), st) == E_NULL
    assert lib.shdr_pair_moments_f32(P(x), P(x), n, h, w, 1, o[0], o[1], o[2], None, st) == E_NULL
    assert lib.shdr_hdr_metrics_f32(P(x), None, n, h, w, 5000.0, o[0], o[1], o[2], o[3], o[4], o[5], o[6], P(ws), st) == E_NULL
    assert lib.shdr_hdr_metrics_f32(P(x), P(x), n, h, w, 5000.0, o[0], o[1], o[2], o[3], o[4], o[5], None, P(ws), st) == E_NULL
    assert lib.shdr_pair_moments_f32(P(x), P(x), n, h, w, 1, o[0], o[1], o[2], P(ws, 4), st) == E_ALIGN
    assert lib.shdr_hdr_metrics_f32(P(x), P(x), n, h, w, 5000.0, o[0], o[1], o[2], o[3], o[4], o[5], o[6], P(ws, 4), st) == E_ALIGN
    ub, u8 = guarded(n * h * w * 3 // 4 + 1)
    assert lib.shdr_tonemap_u8_f32(P(x), None, o[2], P(u8), n, 10, w, 5000.0, 0, st) == E_SHAPE
    assert lib.shdr_tonemap_u8_f32(P(x), None, o[2], P(u8), n, h, w, -1.0, 0, st) == E_SHAPE
    assert lib.shdr_tonemap_u8_f32(None, None, o[2], P(u8), n, h, w, 5000.0, 0, st) == E_NULL
    assert lib.shdr_tonemap_u8_f32(P(x), None, None, P(u8), n, h, w, 5000.0, 0, st) == E_NULL
    assert lib.shdr_metrics_workspace_bytes(n, 10, w) == E_SHAPE
    untouched(wsb, "workspace")
    untouched(ub, "tonemap output")
    for b, _ in out:
        untouched(b, "metric output")
