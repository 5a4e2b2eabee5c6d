"""float64 NumPy restatement of the validation metrics (include/shdr.h "validation metrics", csrc/metrics.hip): the reference the
device kernels are tested against.  Explicit separable loops, no scipy.

One choice is stated here because the arithmetic depends on it: the mean-normalisation scale 0.5 / (1e-6 + mean) multiplies float32
pixels on the device (as K.mean_norm does), so it IS a float32 number -- the mean and the quotient are taken in float64 and the
scale is rounded to float32 once.  Everything after that is float64; in particular peak = scale * max(gt) is the exact product of
two float32 numbers.
"""
import numpy as np

C1, C2 = 1e-4, 9e-4          # (0.01 L)^2, (0.03 L)^2 with L = 1


def gaussian_window(size=11, sigma=1.5):
    x = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


def filter_valid(a, g):
    """separable correlation of a [H, W] with the window g x g, valid positions only: [H - k + 1, W - k + 1]"""
    a = np.asarray(a, dtype=np.float64)
    k = g.size
    h, w = a.shape
    t = np.zeros((h, w - k + 1))
    for i in range(k):
        t += g[i] * a[:, i:i + w - k + 1]
    o = np.zeros((h - k + 1, w - k + 1))
    for i in range(k):
        o += g[i] * t[i:i + h - k + 1]
    return o


def ssim(x, y):
    """mean SSIM of two [H, W] planes with dynamic range 1: weighted population variances and covariance over valid windows"""
    g = gaussian_window()
    mx, my = filter_valid(x, g), filter_valid(y, g)
    vx = filter_valid(x * x, g) - mx * mx
    vy = filter_valid(y * y, g) - my * my
    cxy = filter_valid(x * y, g) - mx * my
    s = ((2.0 * mx * my + C1) * (2.0 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return float(s.mean())


def scale_of(img, normalise):
    """0.5 / (1e-6 + mean(img)) as a float32 number, or 1"""
    if not normalise:
        return 1.0
    return float(np.float32(0.5 / (1e-6 + np.asarray(img, dtype=np.float64).mean())))


def tone(x, peak, mu=5000.0):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log1p(mu * np.minimum(x / peak, 1.0)) / np.log1p(mu)


def logc(x):
    return np.log1p(10.0 * x) / np.log(11.0)


def hdr_metrics_one(pred, gt, normalise=True, mu=5000.0):
    """one image pair [H, W, 3] -> dict of Python floats"""
    pred, gt = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    sp, sg = scale_of(pred, normalise), scale_of(gt, normalise)
    p, g = np.maximum(sp * pred, 0.0), np.maximum(sg * gt, 0.0)
    peak = float(g.max())
    tp, tg = tone(p, peak, mu), tone(g, peak, mu)
    with np.errstate(divide="ignore", invalid="ignore"):
        mse_l = float(np.float64(((p - g) ** 2).mean()) / np.float64(peak * peak))
    return dict(mse_l=mse_l, mse_mu=float(((tp - tg) ** 2).mean()), l1_logc=float(np.abs(logc(p) - logc(g)).mean()),
                ssim_mu=float(np.mean([ssim(tp[..., c], tg[..., c]) for c in range(3)])), peak=peak, scale_pred=sp, scale_gt=sg)


def hdr_metrics(pred, gt, normalise=True, mu=5000.0):
    """[N, H, W, 3] pairs -> dict of float64 arrays [N]"""
    rows = [hdr_metrics_one(p, g, normalise, mu) for p, g in zip(pred, gt)]
    return {k: np.array([r[k] for r in rows], dtype=np.float64) for k in rows[0]}


def tonemap_value(x, peak=None, reverse_channels=False, mu=5000.0, scale=None):
    """[H, W, 3] -> float64: 255 * T(max(scale * x, 0))^(1/2.2) before the rounding to a code, and T itself; scale None -> 1,
    peak None -> the scaled image's maximum"""
    x = np.asarray(x, dtype=np.float64)
    if scale is not None:
        x = float(scale) * x
    x = np.maximum(x, 0.0)
    if reverse_channels:
        x = x[..., ::-1]
    peak = float(x.max()) if peak is None else float(peak)
    t = tone(x, peak, mu)
    return 255.0 * t ** (1.0 / 2.2), t


def tonemap_u8(x, peak=None, reverse_channels=False, mu=5000.0, scale=None):
    """[H, W, 3] -> uint8: round(255 * T(max(scale * x, 0))^(1/2.2)); scale None -> 1, peak None -> the scaled image's maximum"""
    return np.rint(tonemap_value(x, peak, reverse_channels, mu, scale)[0]).astype(np.uint8)


# ---- exact inputs (tests/test_gpu_metrics_exact.py) ---------------------------------------------------------------------------------
TAPS = 11
HALO = TAPS - 1


def ownership_classes(h, w, th, tw):
    """[h, w] int: the class 5 * cy + cx of a pixel in the tiling of csrc/metrics.hip (a tile of th x tw windows stages
    (th + 10) x (tw + 10) pixels).  Per axis: 4 the band of 10 pixels beyond the last window, 1 the first staged line of a tile,
    2 the last line a tile owns, 3 the last line a tile stages (owned by the next tile), 0 the interior."""
    def axis(n, t):
        i = np.arange(n)
        c = np.zeros(n, dtype=np.int64)
        c[(i % t == (t + HALO - 1) % t) & (i >= t + HALO - 1)] = 3
        c[i % t == t - 1] = 2
        c[i % t == 0] = 1
        c[i >= n - HALO] = 4
        return c
    return 5 * axis(h, th)[:, None] + axis(w, tw)[None, :]


def exact_pair(shape, th, tw, seed):
    """(pred, gt, delta) float32 [N, H, W, 3] on which mse_l has no rounding: gt holds multiples of 2^-10 in [2^-4, 1] with an exact
    1.0 per image (peak = 1 without normalisation; image 0 has it at its LAST element), pred = gt + delta with delta in
    +-{2^-4, 2^-6} chosen per image by the ownership class of the pixel.  Every p - g and its square is exact in float32 and every
    sum of them in float64, in any order."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    gt = rng.integers(64, 1025, size=(n, h, w, 3)).astype(np.float64) / 1024.0
    cls = ownership_classes(h, w, th, tw)
    delta = np.empty((n, h, w, 3))
    for i in range(n):
        table = rng.choice([2.0 ** -4, -2.0 ** -4, 2.0 ** -6, -2.0 ** -6], size=25)
        delta[i] = table[cls][:, :, None]
        gt[i].reshape(-1)[-1 if i == 0 else int(rng.integers(0, h * w * 3))] = 1.0
    pred = gt + delta
    out = []
    for a in (pred, gt, delta):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
        out.append(a.astype(np.float32))
    assert pred.min() >= 0.0 and gt.min() >= 2.0 ** -4 and (gt.max(axis=(1, 2, 3)) == 1.0).all()
    return tuple(out)
