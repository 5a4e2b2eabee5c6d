"""CPU tests of the validation metrics: the float64 reference (tests/metrics_ref.py) is pinned by closed forms and by an
independent convolution, and the C ABI refuses bad arguments on the host.  No kernel is launched here."""
import ctypes
import math

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import quantised_image


def _pair(seed=0, hw=(27, 43)):
    rng = np.random.default_rng(seed)
    gt = quantised_image(rng, hw + (3,)) * rng.uniform(1.0, 4.0, hw + (3,))
    pred = np.clip(gt + 0.05 * rng.standard_normal(gt.shape), 0.0, None)
    return pred, gt


@pytest.mark.parametrize("normalise", [False, True])
def test_identical_images(normalise):
    _, gt = _pair(1)
    m = R.hdr_metrics_one(gt, gt, normalise)
    assert m["ssim_mu"] == 1.0
    assert m["mse_l"] == 0.0 and m["mse_mu"] == 0.0 and m["l1_logc"] == 0.0


def test_constant_images_have_closed_forms():
    c, d = 0.7, 0.05
    gt, pred = np.full((15, 17, 3), c), np.full((15, 17, 3), c + d)
    m = R.hdr_metrics_one(pred, gt, normalise=False)
    assert m["peak"] == c and m["scale_pred"] == 1.0 and m["scale_gt"] == 1.0
    assert m["mse_l"] == pytest.approx((d / c) ** 2, rel=1e-12)
    # pred >= peak everywhere: T(pred) = 1 = T(gt) -> no tone-mapped error at all
    assert m["mse_mu"] == 0.0
    assert m["l1_logc"] == pytest.approx(R.logc(c + d) - R.logc(c), rel=1e-12)
    # below the peak: constant planes have zero variance, SSIM is its luminance term
    pred = np.full((15, 17, 3), c - d)
    m = R.hdr_metrics_one(pred, gt, normalise=False)
    mx, my = float(R.tone(c - d, c)), 1.0
    assert m["mse_mu"] == pytest.approx((mx - my) ** 2, rel=1e-12)
    assert m["ssim_mu"] == pytest.approx((2 * mx * my + R.C1) / (mx * mx + my * my + R.C1), abs=1e-12)


def test_ssim_is_symmetric():
    pred, gt = _pair(2)
    peak = max(pred.max(), gt.max())                 # a shared peak: both orders see the same tone curve
    a, b = R.tone(pred[..., 0], peak), R.tone(gt[..., 0], peak)
    assert R.ssim(a, b) == pytest.approx(R.ssim(b, a), abs=1e-15)
    assert 0.0 < R.ssim(a, b) < 1.0


def test_separable_window_matches_conv2d():
    rng = np.random.default_rng(3)
    a = rng.random((27, 43))
    g = R.gaussian_window()
    assert g.sum() == pytest.approx(1.0, abs=1e-15) and g.size == 11 and g[5] == g.max()
    assert g[4] / g[5] == pytest.approx(math.exp(-1.0 / (2 * 1.5 ** 2)), rel=1e-14)
    w2 = torch.from_numpy(np.outer(g, g))[None, None]
    ref = torch.nn.functional.conv2d(torch.from_numpy(a)[None, None], w2)[0, 0].numpy()
    got = R.filter_valid(a, g)
    assert got.shape == (17, 33) == ref.shape
    assert np.abs(got - ref).max() <= 1e-12


def test_normalisation_makes_metrics_scale_invariant():
    """normalise=True: pred * 7.3 changes the normalised image only through the 1e-6 in 0.5 / (1e-6 + mean) and the float32 rounding
    of the two scales.  p' = p (1 + e) with
        |e| <= 1e-6 * 6.3 / (7.3 * mean(pred)) + 2 * 2^-24 =: eps.
    Propagated bounds (only pred moves; x d/dx of logc and of T are at most 1 / ln 11 and 1 / ln(1 + mu) =: t):
        l1_logc : eps / ln 11
        mse_mu  : 2 t eps + (t eps)^2                                  (|T(p) - T(g)| <= 1)
        mse_l   : (2 eps mean(|p - g| p) + eps^2 mean(p^2)) / peak^2
        ssim_mu : with eta = t eps the window mean of T(p) moves by <= eta, its variance by <= 2 sigma_x eta + eta^2, the covariance
                  by <= sigma_y eta.  The luminance term has |dL/dmu_x| <= 2 (mu_x + mu_y) / (mu_x^2 + mu_y^2 + C1) <= sqrt(2 / C1),
                  the contrast term moves by <= (2 (sigma_x + sigma_y) eta + eta^2) / (sigma_x^2 + sigma_y^2 + C2)
                  <= sqrt(2 / C2) eta + eta^2 / C2; both terms are at most 1 in magnitude."""
    pred, gt = _pair(4)
    a, b = R.hdr_metrics_one(pred, gt, True), R.hdr_metrics_one(pred * 7.3, gt, True)
    eps = 1e-6 * 6.3 / (7.3 * pred.mean()) + 2.0 * 2.0 ** -24
    t = 1.0 / math.log1p(5000.0)
    eta = t * eps
    p, g = a["scale_pred"] * pred, a["scale_gt"] * gt
    slack = 1e-13                                                       # float64 arithmetic of the reference itself
    assert abs(b["scale_pred"] * 7.3 / a["scale_pred"] - 1.0) <= eps
    assert b["scale_gt"] == a["scale_gt"] and b["peak"] == a["peak"]
    assert abs(b["l1_logc"] - a["l1_logc"]) <= eps / math.log(11.0) + slack
    assert abs(b["mse_mu"] - a["mse_mu"]) <= 2 * eta + eta * eta + slack
    assert abs(b["mse_l"] - a["mse_l"]) <= (2 * eps * (np.abs(p - g) * p).mean() + eps * eps * (p * p).mean()) / a["peak"] ** 2 + slack
    assert abs(b["ssim_mu"] - a["ssim_mu"]) <= (math.sqrt(2 / R.C1) + math.sqrt(2 / R.C2)) * eta + eta * eta / R.C2 + slack
    # and without the normalisation the metrics do move
    assert abs(R.hdr_metrics_one(pred * 7.3, gt, False)["mse_l"] - R.hdr_metrics_one(pred, gt, False)["mse_l"]) > 1.0


def test_tonemap_reference_end_points():
    x = np.zeros((11, 11, 3))
    x[0, 0] = (0.0, 2.0, 5.0)
    y = R.tonemap_u8(x)
    assert y[0, 0, 2] == 255 and y[0, 0, 0] == 0 and 0 < y[0, 0, 1] < 255
    assert np.array_equal(R.tonemap_u8(x, reverse_channels=True), y[..., ::-1])


def test_tonemap_reference_scale_and_value():
    """the `scale` argument multiplies before the clamp; tonemap_u8 is the rounding of tonemap_value"""
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.5, 5.0, (11, 12, 3))
    assert np.array_equal(R.tonemap_u8(x, peak=3.0, scale=0.75), R.tonemap_u8(0.75 * x, peak=3.0))
    assert np.array_equal(R.tonemap_u8(x, scale=2.0), R.tonemap_u8(x))                 # peak None follows the scaled image
    assert np.array_equal(R.tonemap_u8(x, peak=3.0, scale=-1.0), R.tonemap_u8(-x, peak=3.0))
    val, t = R.tonemap_value(x, 3.0, True, 5000.0, 0.75)
    assert np.array_equal(np.rint(val).astype(np.uint8), R.tonemap_u8(x, 3.0, True, 5000.0, 0.75))
    assert np.array_equal(val, 255.0 * t ** (1.0 / 2.2)) and t.min() == 0.0 and t.max() == 1.0
    # the law of the GPU test: the share of values within k * 2^-24 (relative) of a rounding tie stays far below its 0.5 % condition
    x = rng.integers(0, 1025, size=(2, 300, 300, 3)) / 1024.0 * rng.uniform(1.0, 4.0, (2, 300, 300, 3))
    val, _ = R.tonemap_value(x.astype(np.float32), 3.0)
    tie = np.abs(val - (np.floor(val) + 0.5))
    for k, share in ((16, 0.001), (64, 0.004)):
        assert (tie <= val * k * 2.0 ** -24).mean() <= share


def test_exact_pair_and_ownership_classes():
    th, tw = 16, 32
    cls = R.ownership_classes(49, 83, th, tw)
    assert cls.shape == (49, 83) and set(np.unique(cls // 5)) == {0, 1, 2, 3, 4} == set(np.unique(cls % 5))
    rows = (cls // 5)[:, 0].tolist()
    assert rows[0] == 1 and rows[15] == 2 and rows[16] == 1 and rows[25] == 3 and rows[31] == 2 and rows[38] == 0
    assert rows[39:] == [4] * 10 and rows[9] == 0 and rows[41 - 16] == 3
    cols = (cls % 5)[0].tolist()
    assert cols[0] == 1 and cols[31] == 2 and cols[32] == 1 and cols[41] == 3 and cols[72] == 0 and cols[73:] == [4] * 10
    assert set(np.unique(R.ownership_classes(11, 11, th, tw))) == {6, 9, 21, 24}
    pred, gt, delta = R.exact_pair((3, 27, 43), th, tw, seed=5)
    assert pred.dtype == gt.dtype == np.float32 and gt[0].reshape(-1)[-1] == 1.0
    assert set(np.abs(delta).ravel().tolist()) == {2.0 ** -4, 2.0 ** -6}
    assert np.array_equal(pred.astype(np.float64) - gt.astype(np.float64), delta.astype(np.float64))
    m = R.hdr_metrics(pred, gt, normalise=False)
    assert np.array_equal(m["peak"], np.ones(3)) and np.array_equal(m["scale_gt"], np.ones(3))
    # the reference's own mean is exact: multiples of 2^-12 below 2^53 add without rounding in any order
    assert np.array_equal(m["mse_l"], (delta.astype(np.float64) ** 2).sum(axis=(1, 2, 3)) / (27 * 43 * 3.0))
    # normalised: the mean is the exact sum over the count, the scale its float32 rounding
    n = R.hdr_metrics(pred, gt, normalise=True)
    mean = gt.astype(np.float64).sum(axis=(1, 2, 3)) / (27 * 43 * 3.0)
    assert np.array_equal(n["scale_gt"], (0.5 / (1e-6 + mean)).astype(np.float32).astype(np.float64))
    assert np.array_equal(n["peak"], n["scale_gt"] * 1.0)


def test_reference_of_a_black_ground_truth():
    """peak 0: mse_l is inf, everything that goes through T(0 / 0) is NaN, the loss stays finite -- what csrc/metrics.hip must
    report for such an image (tests/test_gpu_metrics_exact.py)"""
    pred, _ = _pair(6)
    with np.errstate(all="ignore"):
        m = R.hdr_metrics_one(pred, np.zeros_like(pred), normalise=False)
    assert m["peak"] == 0.0 and m["mse_l"] == np.inf and np.isnan(m["mse_mu"]) and np.isnan(m["ssim_mu"])
    assert np.isfinite(m["l1_logc"]) and m["l1_logc"] > 0.0


def test_no_cpu_fallback(shdr):
    x = torch.rand(1, 16, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shdr._ops.hdr_metrics(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shdr._ops.tonemap_u8(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shdr.metrics.Evaluator().update(x, x)
    assert shdr._ops.METRICS_TILE == (16, 32)


def test_host_validation(shdr):
    """bad shapes and null pointers are refused on the host, before any launch"""
    lib = shdr._lib.load()
    buf = np.zeros(64, dtype=np.float64)                       # never dereferenced: the calls return before a launch
    p = ctypes.c_void_p(buf.ctypes.data)
    E_SHAPE, E_NULL = -1, -5
    for n, h, w in ((1, 10, 32), (1, 32, 10), (0, 32, 32), (-1, 32, 32)):
        assert lib.shdr_pair_moments_f32(p, p, n, h, w, 1, p, p, p, p, None) == E_SHAPE
        assert lib.shdr_hdr_metrics_f32(p, p, n, h, w, 5000.0, p, p, p, p, p, p, p, p, None) == E_SHAPE
        assert b"H >= 11" in lib.shdr_last_error()
        assert lib.shdr_tonemap_u8_f32(p, None, p, p, n, h, w, 5000.0, 0, None) == E_SHAPE
        assert lib.shdr_metrics_workspace_bytes(n, h, w) == E_SHAPE
    assert lib.shdr_pair_moments_f32(None, p, 1, 32, 32, 1, p, p, p, p, None) == E_NULL
    assert lib.shdr_pair_moments_f32(p, p, 1, 32, 32, 1, p, p, p, None, None) == E_NULL
    assert lib.shdr_hdr_metrics_f32(p, None, 1, 32, 32, 5000.0, p, p, p, p, p, p, p, p, None) == E_NULL
    assert lib.shdr_hdr_metrics_f32(p, p, 1, 32, 32, 5000.0, p, p, p, p, p, p, None, p, None) == E_NULL
    assert lib.shdr_tonemap_u8_f32(None, None, p, p, 1, 32, 32, 5000.0, 0, None) == E_NULL
    assert lib.shdr_tonemap_u8_f32(p, None, None, p, 1, 32, 32, 5000.0, 0, None) == E_NULL
    # the workspace holds 4 doubles per block of the larger of the two partial tables
    th, tw = shdr._ops.METRICS_TILE
    assert lib.shdr_metrics_workspace_bytes(1, 11, 11) == 32
    assert lib.shdr_metrics_workspace_bytes(3, 2 * th + 10, 3 * tw + 11) == 3 * (2 * 4) * 32
    assert lib.shdr_metrics_workspace_bytes(16, 512, 512) == 16 * 32 * 16 * 32
