"""References of the camera-simulator kernels (csrc/camera.hip) for tests/test_gpu_camera_elem.py, and the wrong models that
tests/test_camera.py uses to show that those tests can fail.  TEST INFRASTRUCTURE ONLY.

`expose64` is joint_training.py:30-43 in float64 on the random stream of the kernel.  Only the steps whose fp32 result IEEE 754
fixes stay in fp32, so that both sides start from the same numbers: the two conversions of 24 random bits to (0, 1), the angle
2 pi_f32 * u2, the two noise levels and x = hdr * t.  log, sqrt, cos, sin and every later product and sum are float64.  (With u1 in
float64 the comparison would be meaningless near u1 -> 1, where log(u1) has lost all but a few bits of u1's own rounding.)

`jpeg_model` is oracle.camera.jpeg_round_trip (pinned against libjpeg in tests/test_camera.py) behind the 8-bit quantisation of
joint_training.py:46-47, with one switch per wrong model."""
import numpy as np

from oracle import camera as O

f32 = np.float32
TWO_PI_F32 = f32(6.283185307179586)


def expose64(hdr, t, seed, per_sample_sigma=False, swap_z=False, clip_first=False):
    """hdr [N, H, W, 3], t [N] -> (hdr_t, clipped, scale) in float64; scale = |x| + (sigma_s |x| + sigma_c) * rad is the size of the
    terms of each element's sum, the unit of the per-element bound.  The keywords select the wrong models."""
    hdr = np.asarray(hdr, dtype=f32)
    n = hdr.shape[0]
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    e = np.arange(hdr.size, dtype=np.uint64)
    zero = np.zeros_like(e)
    r = O.philox4x32_10(np.stack([e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), zero, zero], axis=-1), key)
    u1 = (r[:, 0] >> 8).astype(f32) * f32(2.0 ** -24) + f32(2.0 ** -25)
    u2 = (r[:, 1] >> 8).astype(f32) * f32(2.0 ** -24) + f32(2.0 ** -25)
    ang = (TWO_PI_F32 * u2).astype(np.float64)                                 # the fp32 product, then float64
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    z0, z1 = (rad * np.cos(ang)).reshape(hdr.shape), (rad * np.sin(ang)).reshape(hdr.shape)
    if swap_z:
        z0, z1 = z1, z0
    sc = np.arange(n * 3, dtype=np.uint64)
    if per_sample_sigma:
        sc = sc // np.uint64(3) * np.uint64(3)
    s = O.philox4x32_10(np.stack([sc, np.zeros_like(sc), np.zeros_like(sc), np.ones_like(sc)], axis=-1), key)
    sigma_s = (f32(0.08 / 6.0) * ((s[:, 0] >> 8).astype(f32) * f32(2.0 ** -24))).astype(np.float64).reshape(n, 1, 1, 3)
    sigma_c = (f32(0.005) * ((s[:, 1] >> 8).astype(f32) * f32(2.0 ** -24))).astype(np.float64).reshape(n, 1, 1, 3)
    x = (hdr * np.asarray(t, dtype=f32).reshape(n, 1, 1, 1)).astype(np.float64)
    v = x + z0 * (sigma_s * x) + sigma_c * z1
    if clip_first:
        v = np.maximum(np.minimum(v, 1.0), 0.0)
        clipped = v
    else:
        v = np.maximum(v, 0.0)
        clipped = np.minimum(v, 1.0)
    scale = np.abs(x) + (sigma_s * np.abs(x) + sigma_c) * rad.reshape(hdr.shape)
    return v, clipped, scale


def quantise_u8(x, half_away=False):
    """tf.round(x * 255) in fp32 (half to even), clipped to [0, 255]"""
    p = np.asarray(x, dtype=f32) * f32(255.0)
    r = np.sign(p) * np.floor(np.abs(p) + f32(0.5)) if half_away else np.rint(p)
    return np.clip(r, 0, 255).astype(np.uint8)


def _up_box(p):
    return p.repeat(2, axis=0).repeat(2, axis=1)


def _up_fancy(p):
    """jdsample.c h2v2_fancy_upsample, edges replicated"""
    ph, pw = p.shape
    pad = np.pad(p, 1, mode="edge")
    out = np.empty((2 * ph, 2 * pw), dtype=np.int64)
    for dy in (0, 1):
        col = 3 * pad[1:-1] + (pad[0:-2] if dy == 0 else pad[2:])
        out[dy::2, 0::2] = (3 * col[:, 1:-1] + col[:, 0:-2] + 8) >> 4
        out[dy::2, 1::2] = (3 * col[:, 1:-1] + col[:, 2:] + 7) >> 4
    return out


def _up_fancy_per_mcu(p):
    out = np.empty((2 * p.shape[0], 2 * p.shape[1]), dtype=np.int64)
    for y in range(0, p.shape[0], 8):
        for x in range(0, p.shape[1], 8):
            out[2 * y:2 * y + 16, 2 * x:2 * x + 16] = _up_fancy(p[y:y + 8, x:x + 8])
    return out


def jpeg_model(ldr, quality, half_away=False, high_scale_everywhere=False, luma_for_chroma=False, upsample="fancy"):
    """float [H, W, 3] -> uint8 [H, W, 3]: 8-bit quantisation, then the baseline-JPEG round trip, put together from the oracle's
    stages.  With the default keywords it equals O.jpeg_round_trip(quantise_u8(ldr), quality) (tests/test_camera.py); every keyword
    switches ONE step to a plausible wrong rule."""
    rgb = quantise_u8(ldr, half_away).astype(np.int64)
    h, w, _ = rgb.shape
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    half, off = 1 << 15, 128 << 16
    fix = O._fix16
    y = (fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.50000) * b + off + half - 1) >> 16
    cr = (fix(0.50000) * r - fix(0.41869) * g - fix(0.08131) * b + off + half - 1) >> 16

    def down(p):
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        return (s + (1 + (np.arange(w // 2) & 1))[None, :]) >> 2
    q = min(max(int(quality), 1), 100)
    scale = 200 - 2 * q if (q >= 50 or high_scale_everywhere) else 5000 // q
    ql, qc = (np.clip((t * scale + 50) // 100, 1, 255).astype(np.int32) for t in (O.LUMA_Q, O.CHROMA_Q))
    if luma_for_chroma:
        qc = ql
    up = dict(fancy=_up_fancy, box=_up_box, per_mcu=_up_fancy_per_mcu)[upsample]
    y2 = O._code_plane(y, ql)
    cbu, cru = up(O._code_plane(down(cb), qc)) - 128, up(O._code_plane(down(cr), qc)) - 128
    rr = y2 + ((fix(1.40200) * cru + half) >> 16)
    gg = y2 + ((-fix(0.34414) * cbu + half - fix(0.71414) * cru) >> 16)
    bb = y2 + ((fix(1.77200) * cbu + half) >> 16)
    return np.clip(np.stack([rr, gg, bb], axis=-1), 0, 255).astype(np.uint8)


def census(jpeg_u8, bright=249, dark=6):
    """(#grey >= bright, #grey <= dark) of one image [H, W, 3]"""
    gray = O.rgb_to_gray_u8(jpeg_u8)
    return int((gray >= bright).sum()), int((gray <= dark).sum())


def loss_mask(jpeg_u8, bright=249, dark=6, inclusive=False):
    """joint_training.py:54-63 for one image: 0 where MORE than 256 * 256 * 0.5 pixels are >= 249 or <= 6 grey levels"""
    over, under = census(jpeg_u8, bright, dark)
    hit = (over >= 32768 or under >= 32768) if inclusive else (over > 32768 or under > 32768)
    return 0.0 if hit else 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_camera_elem.py, shared with tests/test_camera.py (the wrong models must fail AT THESE INPUTS)
# ---------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
# Per-element bound of camera_expose against expose64: |got - ref| <= K_EXPOSE u scale.  MEASURED against the float64 reference on
# an MI355X: worst err / (u scale) = 3.256 over the four cases (at 2 x 300 x 300); K_EXPOSE is four times that (the device's logf /
# cosf / sinf round the last place differently from any host library).  It must stay <= 32 to mean anything.
K_EXPOSE = 13.1

EXPOSE_CASES = [(1, 1, 1), (1, 5, 17), (3, 40, 56), (2, 300, 300)]        # N, H, W; the last has 540000 elements


def expose_input(case):
    n, h, w = case
    rng = np.random.default_rng([n, h, w])
    hdr = (rng.random((n, h, w, 3)) ** 3 * 4).astype(np.float32)
    hdr[:, ::3] = 0                                                       # rows of zeros: v = max(sigma_c z1, 0) there
    t = np.array([0.5, 0.0, 3.0], dtype=np.float32)[:n] if n > 1 else np.array([1.5], dtype=np.float32)
    if n == 2:
        t = np.array([2.0, 0.25], dtype=np.float32)
    return hdr, t, 0x1234567890 + n * h * w


def ties():
    """fp32 x whose fp32 product x * 255 is exactly k + 0.5: [(x, k)], found by search around (k + 0.5) / 255"""
    found = []
    for k in range(255):
        x = f32((k + 0.5) / 255.0)
        for _ in range(3):
            x = np.nextafter(x, f32(0))
        for _ in range(7):
            if x * f32(255.0) == f32(k + 0.5):
                found.append((x, k))
                break
            x = np.nextafter(x, f32(1))
    return found


JPEG_SIZES = [(16, 16), (16, 48), (48, 16), (32, 32), (528, 512)]
JPEG_QUALITIES = [[1, 50, 100], [2, 49, 51], [10, 75, 89]]
JPEG_CLAMPED = [([0, -3, 101], [1, 1, 100]), ([1000, -2 ** 31, 2 ** 31 - 1], [100, 1, 100])]


def jpeg_contents(h, w, seed):
    """five float32 images [H, W, 3]: white noise, smooth ramp, 0/255 checker (drives the IDCT into its range clamp), flat, and one
    OFF the 8-bit grid: values below 0 and above 1 and every tie x * 255 = k + 0.5"""
    rng = np.random.default_rng([h, w, seed])
    yy, xx = np.mgrid[0:h, 0:w]
    noise = rng.integers(0, 256, size=(h, w, 3)).astype(f32) / f32(255)
    ramp = np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1), (xx + yy + seed) % 256], -1).astype(f32) / f32(255)
    checker = np.repeat((((yy + xx + seed) & 1) * 255)[..., None], 3, axis=-1).astype(f32) / f32(255)
    checker[..., 1] = checker[::-1, :, 1]
    flat = np.broadcast_to(np.array([37 + seed, 200, 255], dtype=f32) / f32(255), (h, w, 3)).copy()
    off = (rng.random((h, w, 3)) * 1.6 - 0.3).astype(f32)
    t = np.array([x for x, _ in ties()], dtype=f32)
    flatview = off.reshape(-1)
    pos = rng.permutation(flatview.size)[:len(t)]
    flatview[pos] = t[:len(pos)]
    return dict(noise=noise, ramp=ramp, checker=checker, flat=flat, off=off)


def jpeg_batches(h, w):
    """[(ldr float32 [3, H, W, 3], qualities [3])]: different images per sample, different qualities in one batch"""
    if h * w > 65536:
        c = jpeg_contents(h, w, 0)
        return [(np.stack([c["noise"], c["off"], c["ramp"]]), [2, 50, 100])]
    out = []
    names = [("noise", "ramp", "checker"), ("flat", "off", "noise"), ("checker", "off", "ramp")]
    for i, (q, nm) in enumerate(zip(JPEG_QUALITIES, names)):
        c = jpeg_contents(h, w, i)
        out.append((np.stack([c[k] for k in nm]), q))
    return out


def _grey(h, w, level):
    return np.full((h, w, 3), level, dtype=np.uint8)


def mask_cases():
    """name -> (uint8 image, (#>= 249, #<= 6) after a quality-100 round trip, mask).  Flat 8 x 8 luma blocks survive quality 100
    unchanged, so the counts sit exactly at the threshold 256 * 256 * 0.5 = 32768 and one pixel above it."""
    cases = {}
    a = _grey(256, 256, 248)
    a[:128] = 249
    cases["bright_at"] = (a, (32768, 0), 1.0)
    b = a.copy()
    b[128:136, 8:16] = 240
    b[131, 11] = 255
    cases["bright_above"] = (b, (32769, 0), 0.0)
    c = _grey(256, 256, 7)
    c[:128] = 6
    cases["dark_at"] = (c, (0, 32768), 1.0)
    d = c.copy()
    d[128:136, 8:16] = 16
    d[131, 11] = 0
    cases["dark_above"] = (d, (0, 32769), 0.0)
    e = _grey(528, 512, 248)                     # 270336 pixels: rows 512.. are the finish kernel's second grid-stride trip
    e[464:] = 249                                # 64 rows = 32768 pixels, 8192 of them in the second trip
    e[0:8, 8:16] = 240
    e[3, 11] = 255
    cases["second_trip"] = (e, (32769, 0), 0.0)
    cases["small_white"] = (_grey(64, 64, 255), (4096, 0), 1.0)         # the threshold is the constant, not half the image
    return cases
