"""Float64 references of the image plumbing kernels (csrc/imageio.hip), written from the definitions of the operations and not from
the kernels: tests/test_gpu_imageio_elem.py compares the device with them element by element, tests/test_imageio_ref.py checks on
the CPU that the comparison can fail (the WRONG_* models: the reference with one plausible error each).  TEST INFRASTRUCTURE ONLY.

`cubic` is OpenCV's INTER_CUBIC (resize.cpp): the source coordinate of destination index d is (float)((d + 0.5) * scale - 0.5) with
scale = 1 / (n_out / n_in) in double.  The one rounding to fp32 belongs to the definition, so the fraction t = f - floor(f) (exact in
fp32) is the SAME number here and in the kernel; the weights (interpolateCubic, A = -0.75) of the taps floor(f) - 1 .. floor(f) + 2,
clamped to the image, and all 16 products and their sum are float64 here."""
import numpy as np

A_CV = -0.75


def cubic_axis(n_in, n_out, A=A_CV, first=-1, border="replicate", coord="opencv", ratio=None):
    """(idx [n_out, 4] into the source axis, w [n_out, 4] float64).  The keywords select the wrong models of test_imageio_ref.py;
    ratio = (a, b) takes the scale from a -> b instead of n_in -> n_out."""
    d = np.arange(n_out, dtype=np.float64)
    clamp_to = n_in
    if ratio is not None:
        n_in, n_out = ratio
    if coord == "opencv":
        f = ((d + 0.5) * (1.0 / (np.float64(n_out) / np.float64(n_in))) - 0.5).astype(np.float32)
    elif coord == "fp32":                         # the rule this kernel had before: fp32 scale, fp32 arithmetic
        f = (d.astype(np.float32) + np.float32(0.5)) * np.float32(np.float64(n_in) / n_out) - np.float32(0.5)
    elif coord == "align_corners":
        f = (d * (np.float64(n_in - 1) / max(n_out - 1, 1))).astype(np.float32)
    else:
        raise ValueError(coord)
    s = np.floor(f)
    t = (f - s).astype(np.float64)                # exact in fp32: the same t as the kernel's
    s = s.astype(np.int64)
    w = np.stack([((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A,
                  ((A + 2) * t - (A + 3)) * t * t + 1,
                  ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1], axis=1)
    w = np.concatenate([w, 1.0 - w.sum(axis=1, keepdims=True)], axis=1)
    idx = s[:, None] + first + np.arange(4)[None, :]
    if border == "replicate":
        idx = np.clip(idx, 0, clamp_to - 1)
    elif border == "reflect":                     # -1 -> 0, n -> n - 1, folded as often as a tiny image needs
        idx = np.mod(idx, 2 * clamp_to)
        idx = np.where(idx >= clamp_to, 2 * clamp_to - 1 - idx, idx)
    else:
        raise ValueError(border)
    return idx, w


def cubic(x, out_hw, swap_scales=False, **axis_kw):
    """x [N, H, W, C] -> (y, S, T), each float64 [N, Ho, Wo, C]: the resized tensor, S = sum |cy_i| |cx_j| |x_ij| and T = sum |x_ij|
    over each element's 16 taps (the two scales of the per-element tolerance)"""
    x = np.asarray(x, dtype=np.float64)
    n, h, w, c = x.shape
    ho, wo = out_hw
    iy, cy = cubic_axis(h, ho, ratio=(w, wo) if swap_scales else None, **axis_kw)      # swap_scales: a wrong model
    ix, cx = cubic_axis(w, wo, ratio=(h, ho) if swap_scales else None, **axis_kw)
    y, S, T = (np.zeros((n, ho, wo, c)) for _ in range(3))
    ax = np.abs(x)
    for i in range(4):
        for j in range(4):
            wgt = (cy[:, i, None] * cx[None, :, j])[None, :, :, None]
            y += wgt * x[:, iy[:, i]][:, :, ix[:, j]]
            tap = ax[:, iy[:, i]][:, :, ix[:, j]]
            S += np.abs(wgt) * tap
            T += tap
    return y, S, T


def pad_symmetric(x, pad, repeat_edge=True, pad_hw=None):
    """np.pad(..., 'symmetric') by index arithmetic: out[i] = x[-i - 1] left of the image, x[2n - 1 - i] right of it"""
    x = np.asarray(x)
    n, h, w, c = x.shape
    ph, pw = (pad, pad) if pad_hw is None else pad_hw

    def src(size, p):
        i = np.arange(-p, size + p)
        if repeat_edge:
            return np.where(i < 0, -i - 1, np.where(i >= size, 2 * size - 1 - i, i))
        return np.clip(np.where(i < 0, -i, np.where(i >= size, 2 * size - 2 - i, i)), 0, size - 1)        # 'reflect'
    return x[:, src(h, ph)][:, :, src(w, pw)]


def flip_rot90(x, flip, k, divisor, order="flip_first", clockwise=False, reduce_k=True):
    """per sample: tf.image.rot90(tf.image.flip_left_right(x) if flip else x, k) / divisor, counter-clockwise, k mod 4; by index
    arithmetic: one counter-clockwise quarter turn of a square m is out[i][j] = m[j][S - 1 - i]"""
    x = np.asarray(x, dtype=np.float32)
    n, s, _, c = x.shape
    ii, jj = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    out = np.empty_like(x)

    def turn(m, q):
        if not reduce_k and not 0 <= q <= 3:
            return m
        for _ in range(q % 4):
            m = m[s - 1 - jj, ii] if clockwise else m[jj, s - 1 - ii]
        return m
    for b in range(n):
        m = x[b]
        if order == "flip_first":
            m = turn(m[:, ::-1] if flip[b] else m, int(k[b]))
        else:
            m = turn(m, int(k[b]))
            m = m[:, ::-1] if flip[b] else m
        out[b] = m / np.float32(divisor)
    return out


def u8_to_unit(u8, reverse=False):
    y = np.asarray(u8).astype(np.float32) / np.float32(255)
    return y[..., ::-1] if reverse else y


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_imageio_elem.py, shared with tests/test_imageio_ref.py (which shows on the CPU that every wrong model
# fails AT THESE INPUTS)
# ---------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
LAUNCH_THREADS = 2048 * 256                       # shdr::stream_grid: more work items than this take a second grid-stride trip

# (H, W, Ho, Wo, largest |integer|): every ratio a power of two, so all weights, products and partial sums are exact in fp32
CUBIC_EXACT = [(9, 7, 9, 7, 8), (9, 7, 18, 14, 8), (18, 14, 9, 7, 8), (9, 7, 18, 7, 8), (9, 8, 36, 8, 8), (16, 16, 4, 4, 8),
               (5, 6, 10, 3, 8), (6, 5, 3, 10, 64), (7, 5, 28, 20, 1)]
# (N, H, W, C, Ho, Wo)
CUBIC_GENERAL = [(2, 5, 100, 3, 7, 128), (1, 17, 200, 4, 64, 256), (2, 64, 64, 3, 33, 47), (1, 1, 1, 1, 3, 5), (2, 2, 3, 3, 1, 1),
                 (1, 1, 1408, 3, 1, 1400), (1, 3, 4000, 3, 3, 4032), (1, 420, 420, 3, 421, 419)]
CUBIC_WIDE = [(1, 1, 1408, 3, 1, 1400), (1, 3, 4000, 3, 3, 4032)]


def case_id(case):
    return "x".join(str(v) for v in case)


def cubic_exact_input(case, n, c):
    h, w, _, _, top = case
    rng = np.random.default_rng([h, w, top, n, c])
    return rng.integers(-top, top + 1, size=(n, h, w, c)).astype(np.float32)          # drawn per image and channel: all distinct


def cubic_general_input(case):
    n, h, w, c, _, _ = case
    return np.random.default_rng([n, h, w, c]).standard_normal((n, h, w, c)).astype(np.float32)


# Per-element bound of the fp32 kernel against `cubic`: |got - ref| <= A_TOL u S + B_TOL u T, u = 2^-24 (the derivation is in the
# docstring of tests/test_gpu_imageio_elem.py; nothing in it comes from a run of the kernel).
A_TOL, B_TOL = 9.0, 82.0


def cubic_tol(S, T):
    return (A_TOL * U) * S + (B_TOL * U) * T


def u8_pixels(npix):
    """[npix, 3] uint8; from 256 pixels on every channel holds all 256 values, in a different order per channel"""
    p = np.arange(npix, dtype=np.int64)
    return np.stack([p % 256, (p * 7 + 3) % 256, (255 - p * 3) % 256], axis=1).astype(np.uint8)


PAD_CASES = [(1, 1, 5, 3, 0), (1, 1, 5, 3, 1), (1, 5, 1, 1, 0), (1, 5, 1, 1, 1), (1, 1, 1, 4, 1),
             (2, 9, 7, 1, 0), (2, 9, 7, 3, 1), (2, 9, 7, 4, 7), (2, 7, 9, 3, 7), (2, 4, 4, 3, 4),
             (2, 300, 290, 3, 5)]                 # (N, H, W, C, pad); the last has 558000 output elements


def pad_input(case):
    n, h, w, c, _ = case
    return (np.arange(n * h * w * c, dtype=np.float32) + np.float32(0.5)).reshape(n, h, w, c)


FLIP_ROT = [(f, k) for f in (0, 1) for k in (0, 1, 2, 3, 4, 5, 6, 7, -1)]
FLIP_CASES = [(s, c, d) for s in (1, 2, 7, 12) for c in (1, 3) for d in (255.0, 1.0)] + [(100, 3, 255.0)]      # 18 * 100 * 100 * 3 = 540000


def flip_input(case):
    s, c, _ = case
    n = len(FLIP_ROT)
    x = np.random.default_rng([s, c]).permutation(n * s * s * c).astype(np.float32).reshape(n, s, s, c)      # distinct, exact in fp32
    return x, np.array([f for f, _ in FLIP_ROT], dtype=np.int32), np.array([k for _, k in FLIP_ROT], dtype=np.int32)


def rgbe_pixels():
    """([M, 3] float32 special pixels, list of (row, channel, byte) that the truncating cast must give).  The scale of a pixel with
    maximum v = m 2^e is m * 256 / v = 2^(8 - e) exactly, so a channel at j 2^(e - 8) must give j and the fp32 number below it j - 1."""
    f = np.float32
    px = [[0, 0, 0], [1.0, 0.5, 0.25], [-1.0, 2.0, 1e-35], [1e-33, 0, 0]]
    for k in (-100, -1, 0, 1, 100):
        v = f(2.0) ** f(k)
        for ch, val in enumerate((np.nextafter(v, f(0)), v, np.nextafter(v, f(np.inf)))):
            p = [val * f(0.37), val * f(0.5), val * f(0.999)]
            p[ch] = val
            px.append(p)
    expect = []
    for v, ch in ((f(1.0), 0), (f(1.5), 1), (f(26.0), 2), (np.nextafter(f(2.0), f(0)), 0), (f(2.0) ** f(-60) * f(1.25), 1)):
        m, e = np.frexp(v)
        for j in (1, 2, 77, 127, 128):
            at = f(j) * f(2.0) ** f(int(e) - 8)
            assert at <= v
            p = [at, at, at]
            p[ch] = v
            below = np.nextafter(at, f(0))
            p[(ch + 2) % 3] = below
            expect += [(len(px), (ch + 1) % 3, j), (len(px), (ch + 2) % 3, j - 1)]
            px.append(p)
    t = f(1e-32)
    px += [[t, 0, 0], [0, np.nextafter(t, f(0)), 0], [0, 0, np.nextafter(t, f(1))], [np.nextafter(t, f(0)), t * f(0.5), 0]]
    return np.array(px, dtype=np.float32), expect


def rgbe_input(npix):
    """[npix, 3]: the special pixels first (as many as fit), then radiances over 60 octaves with some negative channels"""
    rng = np.random.default_rng(npix)
    x = ((rng.random((npix, 3)) - 0.05) * np.exp2(rng.integers(-30, 31, size=(npix, 1)))).astype(np.float32)
    sp, _ = rgbe_pixels()
    m = min(npix, len(sp))
    x[:m] = sp[:m]
    return x
