"""float64 NumPy restatement of the gain-map rules (include/shdr.h "gain maps"), written from the rules and not from csrc/gainmap.h:
the reference of tests/test_gainmap_host.py, and the shapes, contents and error figures that the CPU and GPU tests share.

  SDR   the sRGB EOTF of the byte.                     HDR   max(x, 0), NaN -> 0, +inf -> FLT_MAX.
  s     given, or 2^a with a = mean log2 Y_sdr - mean log2 max(Y_hdr, 2^-20) over the pixels whose SDR bytes all lie in [16, 239]
        (Y: Rec.709 luminance of the linear values); no such pixel: s = 1.
  cell  box averages over f x f pixels clipped to the image; g = log2((s hdr + 1/64) / (sdr + 1/64)) clamped to [lo, hi].
  range min, max over the image; max - min < 2^-10 -> max = min + 2^-10.     code  255 (g - min) / (max - min), before rounding.
  apply r = code / 255 sampled bilinearly at u = (x + 0.5) / f - 0.5 clamped to the map; r = r^(1 / gamma); L = min (1 - r) + max r;
        out = max((sdr + offset_sdr) 2^(L w) - offset_hdr, 0).
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24                                   # unit round-off of fp32

# measured by tools/gainmap_sweep.cpp against float64 (DESIGN.md "Gain maps")
E_LOG2_E0 = 1.088e-7        # |log2_poly - log2| over every fp32 mantissa at exponent 0 (the result is z p alone: no exponent is added)
E_LOG2 = 5.649e-7           # ... at the exponents -8 .. 8: every argument whose log2 the range [-4, 8] and the offsets 1/64 let through
E_EXP2 = 9.617e-8           # |exp2_poly / exp2 - 1| on the grid k 2^-16 of [-16, 16]

SHAPES = [(1, 1), (1, 9), (2, 3), (3, 5), (4, 4), (5, 7), (8, 8), (9, 17), (16, 33), (31, 64), (65, 130)]
FACTORS = (1, 2, 4, 8)
CONTENTS = ("noise", "ramp", "constant", "no_qualifying", "specials", "both_ends")


def srgb_table():
    v = np.arange(256, dtype=np.float64) / 255.0
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def sanitise(hdr):
    x = np.asarray(hdr, dtype=np.float64)
    x = np.where(np.isnan(x), 0.0, x)
    return np.minimum(np.maximum(x, 0.0), FLT_MAX)


def luminance(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def alignment(sdr, hdr, reverse=False):
    """(a, count): the log2 of the automatic scale and the number of pixels behind it; a is 0 when none qualifies"""
    h = sanitise(hdr)[..., ::-1] if reverse else sanitise(hdr)
    ok = ((sdr >= 16) & (sdr <= 239)).all(axis=-1)
    n = int(ok.sum())
    if n == 0:
        return 0.0, 0
    ys = luminance(srgb_table()[sdr])[ok]
    yh = np.maximum(luminance(h)[ok], 2.0 ** -20)
    return float(np.log2(ys).mean() - np.log2(yh).mean()), n


def box(x, f):
    """box averages [ceil(H / f), ceil(W / f), C] of x [H, W, C], edge cells clipped to the image"""
    rows = np.add.reduceat(x, np.arange(0, x.shape[0], f), axis=0)
    sums = np.add.reduceat(rows, np.arange(0, x.shape[1], f), axis=1)
    ones = np.ones(x.shape[:2] + (1,))
    count = np.add.reduceat(np.add.reduceat(ones, np.arange(0, x.shape[0], f), axis=0), np.arange(0, x.shape[1], f), axis=1)
    return sums / count


def gains(sdr, hdr, f, s, log2_range=(-4.0, 8.0), reverse=False):
    """(g [h, w, 3] clamped, min, max) with the 2^-10 rule applied to max"""
    h = sanitise(hdr)[..., ::-1] if reverse else sanitise(hdr)
    g = np.log2((box(h * float(s), f) + 1.0 / 64) / (box(srgb_table()[sdr], f) + 1.0 / 64))
    g = np.clip(g, log2_range[0], log2_range[1])
    mn, mx = float(g.min()), float(g.max())
    if mx - mn < 2.0 ** -10:
        mx = mn + 2.0 ** -10
    return g, mn, mx


def ideal_codes(g, mn, mx):
    return 255.0 * (g - mn) / (mx - mn)


def apply(sdr, codes, f, mn, mx, gamma=1.0, offset_sdr=1.0 / 64, offset_hdr=1.0 / 64, weight=1.0):
    """(out [H, W, 3], A): rule 8 in float64; A = (sdr + offset_sdr) 2^(L w), the quantity whose relative error the twin's bound is about.
    codes: uint8 [h, w, 1 or 3]"""
    H, W, _ = sdr.shape
    mh, mw, mc = codes.shape
    r = codes.astype(np.float64) / 255.0
    u = np.clip((np.arange(W) + 0.5) / f - 0.5, 0, mw - 1)
    v = np.clip((np.arange(H) + 0.5) / f - 0.5, 0, mh - 1)
    xa, ya = np.floor(u).astype(int), np.floor(v).astype(int)
    xb, yb = np.minimum(xa + 1, mw - 1), np.minimum(ya + 1, mh - 1)
    fx, fy = (u - xa)[None, :, None], (v - ya)[:, None, None]
    top = r[ya][:, xa] + (r[ya][:, xb] - r[ya][:, xa]) * fx
    bottom = r[yb][:, xa] + (r[yb][:, xb] - r[yb][:, xa]) * fx
    rr = top + (bottom - top) * fy
    if gamma != 1.0:
        rr = np.maximum(rr, 0.0) ** (1.0 / gamma)
    L = mn * (1.0 - rr) + mx * rr
    A = (srgb_table()[sdr] + offset_sdr) * np.exp2(L * weight)
    return np.maximum(A - offset_hdr, 0.0), A


# ---------------------------------------------------------------- the cases that the CPU and the GPU tests share
def content(name, shape, seed):
    """(sdr uint8 [H, W, 3], hdr float32 [H, W, 3] in RGB order) of one content case"""
    rng = np.random.default_rng(seed)
    H, W = shape
    lin = srgb_table()
    if name == "noise":
        sdr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        hdr = lin[sdr] * np.exp2(rng.uniform(-3, 4, (H, W, 3)))
    elif name == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        t = (x + y * W) / max(H * W - 1, 1)
        sdr = np.stack([20 + 200 * t, 230 - 180 * t, 40 + 100 * t], axis=-1).astype(np.uint8)
        hdr = lin[sdr] * (0.5 + 6.0 * t[..., None] ** 2)
    elif name == "constant":
        sdr = np.full((H, W, 3), 117, dtype=np.uint8)
        hdr = np.full((H, W, 3), 0.75)
    elif name == "no_qualifying":
        sdr = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
        hdr = rng.uniform(0, 3, (H, W, 3))
    elif name == "specials":
        sdr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        hdr = lin[sdr] * np.exp2(rng.uniform(-2, 2, (H, W, 3)))
        pick = rng.integers(0, 12, (H, W, 3))
        for k, v in enumerate((0.0, -1.5, np.nan, np.inf, 1e30, -np.inf)):
            hdr[pick == k] = v
    elif name == "both_ends":
        sdr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        hdr = np.where(rng.random((H, W, 3)) < 0.5, 0.0, 4000.0) if H * W > 1 else np.array([[[0.0, 4000.0, 1.0]]])
    else:
        raise ValueError(name)
    return sdr, np.ascontiguousarray(hdr, dtype=np.float32)


def cases(name):
    """every shape and factor with one content; reverse_channels and the scale (None: "auto") alternate so that each shape meets each"""
    out = []
    for si, shape in enumerate(SHAPES):
        for fi, f in enumerate(FACTORS):
            reverse = bool((si + fi) & 1)
            scale = None if (si + (fi >> 1)) & 1 == 0 else 0.25 + 0.5 * fi
            sdr, hdr = content(name, shape, 1000 * si + 10 * fi + CONTENTS.index(name))
            out.append(dict(name="%s-%dx%d-f%d-%s-%s" % (name, shape[0], shape[1], f, "bgr" if reverse else "rgb", "auto" if scale is None else "fixed"),
                            sdr=sdr, hdr=hdr[..., ::-1].copy() if reverse else hdr, factor=f, reverse=reverse, scale=scale))
    return out


def spacing32(v):
    """the distance between neighbouring fp32 numbers at |v|"""
    return float(np.spacing(np.float32(abs(v))))


def round_trip_bound(sdr, hdr, s, mn, mx, J, log2_range=(-4.0, 8.0)):
    """(T, bound) of decode(encode(hdr, sdr)) at f = 1 and w = 1 (tests/test_ultrahdr_container.py has the derivation): T is s * hdr after
    rule 2 and the rule 5 clamp, T = (lin + 1/64) 2^g - 1/64 with g the pixel's clamped gain; hdr in RGB order; J = |decoded map - coded
    map| in codes, per element.  The decoded code is off the real-valued code of g by at most 1/2 + delta + J, L by that times
    (max - min) / 255, the output by the factor 2^dL, and the twin's own apply error comes on top."""
    ln2 = float(np.log(2.0))
    lin = srgb_table()[sdr]
    g = np.clip(np.log2((sanitise(hdr) * s + 1.0 / 64) / (lin + 1.0 / 64)), log2_range[0], log2_range[1])
    A = (lin + 1.0 / 64) * np.exp2(g)
    T = np.maximum(A - 1.0 / 64, 0.0)
    delta = 255.0 / (mx - mn) * 3 * E_LOG2 + 255 * 4 * U
    dL = (0.5 + delta + J) * (mx - mn) / 255.0
    twin = E_EXP2 + ln2 * ((abs(mn) + abs(mx)) * 8 * U + (mx - mn) * 8 * U + 2 * spacing32(max(abs(mn), abs(mx)))) + 4 * U
    return T, A * np.exp2(dL) * ((np.exp2(dL) - 1.0) + twin) + U * T
