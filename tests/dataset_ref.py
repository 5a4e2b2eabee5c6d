"""CPU restatement of the reference's dataset.py pixel path (HDRDataset._hdr_read_resize, PatchHDRDataset.__getitem__) in
float32 numpy, with the RNG calls replaced by drawn parameters.  cv2.resize is restated as OpenCV's generic INTER_LINEAR path
(see csrc/dataset.hip).  Every function also returns, per output value, the largest of its four source taps: the tests'
tolerance is relative to it, which holds across the dynamic range of HDR data."""
import numpy as np


def _axis(dsize, ssize, clamp_weight):
    scale = 1.0 / (dsize / ssize)
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_weight:
        lo, hi = s < 0, s >= ssize - 1
        s[lo], f[lo] = 0, 0
        s[hi], f[hi] = ssize - 1, 0
    return np.clip(s, 0, ssize - 1), np.clip(s + 1, 0, ssize - 1), f


def resize_linear(img, out_hw):
    """cv2.resize(img, (W, H)) with the default INTER_LINEAR on float32 [h, w, c] -> (resized, max of the 4 taps)"""
    img = np.asarray(img, dtype=np.float32)
    h, w, _ = img.shape
    H, W = out_hw
    y0, y1, fy = _axis(H, h, False)
    x0, x1, fx = _axis(W, w, True)
    one = np.float32(1.0)
    gx, gy = (one - fx)[None, :, None], (one - fy)[:, None, None]
    hx = img[:, x0] * gx + img[:, x1] * fx[None, :, None]                     # horizontal pass, every source row
    out = hx[y0] * gy + hx[y1] * fy[:, None, None]
    tap = np.maximum(np.maximum(img[y0][:, x0], img[y0][:, x1]), np.maximum(img[y1][:, x0], img[y1][:, x1]))
    return out.astype(np.float32), np.abs(tap)


def rgbe_bgr(rgbe):
    """uint8 [h, w, 4] RGBE bytes -> float32 BGR [h, w, 3]: byte * 2^(e - 136), e == 0 -> 0 (rgbe_bgr of csrc/dataset.hip).  Exact:
    a byte times a power of two is a float32 number down to the subnormals (e = 1: 2^-135 ... 255 * 2^-135)."""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    e = rgbe[..., 3].astype(np.int32)
    v = np.ldexp(rgbe[..., 2::-1].astype(np.float32), (e - 136)[..., None]).astype(np.float32)
    return np.where((e == 0)[..., None], np.float32(0.0), v)


def half_bits_to_float(h):
    """uint16 IEEE binary16 bit patterns -> float32, in integer arithmetic: +-0, subnormals, +-inf and NaN payloads (not quieted,
    which a hardware conversion would do) are kept -- half_bits_to_float of csrc/exr.hip"""
    h = np.asarray(h, dtype=np.uint16).astype(np.uint32)
    sign, e, m = (h & 0x8000) << 16, (h >> 10) & 0x1F, h & 0x3FF
    normal = sign | ((e + 112) << 23) | (m << 13)
    special = sign | 0x7F800000 | (m << 13)
    sub = sign | (m.astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)
    return np.where(e == 0x1F, special, np.where(e == 0, sub, normal)).astype(np.uint32).view(np.float32)


def clip0(x):
    """the loaders' np.clip(x, 0, None) as the kernel states it: negatives (and -inf) become +0; -0, NaN and +inf pass"""
    return np.where(x < 0, np.float32(0.0), x)


def load(rgb):
    """HDRDataset._hdr_read_resize on a decoded RGB file image (hdr_io.read_hdr): BGR, clip, short side to 512"""
    bgr = np.clip(np.asarray(rgb, dtype=np.float32)[:, :, ::-1], 0, None)
    h, w, _ = bgr.shape
    ratio = max(512 / h, 512 / w)
    return resize_linear(bgr, (round(h * ratio), round(w * ratio)))


def window(img, parity):
    """the 512 crop of PatchHDRDataset.__getitem__ (:214-219)"""
    h, w, _ = img.shape
    if h > w:
        return img[:512] if parity == 0 else img[-512:]
    return img[:, :512] if parity == 0 else img[:, -512:]


def patch(img, idx, S, y0, x0, k, flip0, flip1, mean, is_training=True):
    """PatchHDRDataset.__getitem__(idx) of the resident image of file idx // 2, with `mean` for np.mean of the crop"""
    hdr = window(img, idx % 2)
    hdr = (np.float32(0.5) * hdr / np.float32(np.float32(mean) + np.float32(1e-6))).astype(np.float32)      # _pre_hdr_p2
    if not is_training:
        return hdr, np.abs(hdr)
    hdr, tap = resize_linear(hdr, (S, S))
    if S != 256:
        hdr, tap = hdr[y0:y0 + 256, x0:x0 + 256], tap[y0:y0 + 256, x0:x0 + 256]
    hdr, tap = np.rot90(hdr, k), np.rot90(tap, k)
    if flip0:
        hdr, tap = np.flip(hdr, 0), np.flip(tap, 0)
    if flip1:
        hdr, tap = np.flip(hdr, 1), np.flip(tap, 1)
    return np.ascontiguousarray(hdr), np.ascontiguousarray(tap)


def patch_crop(img, idx, S, y0, x0, k, flip0, flip1, mean, P=256):
    """patch() for a training crop of side P, evaluating only the P rows and P columns of the S x S resize that the crop keeps:
    the same float32 operations in the same order (normalise the taps, horizontal pass, vertical pass), so the values are those of
    patch() bit for bit (tests/test_dataset.py pins that at P = 256)"""
    win = window(img, idx % 2)
    denom = np.float32(np.float32(mean) + np.float32(1e-6))
    r0, r1, fy = (a[y0:y0 + P] for a in _axis(S, 512, False))
    c0, c1, fx = (a[x0:x0 + P] for a in _axis(S, 512, True))
    assert len(r0) == P == len(c0), "crop outside the resized image"
    one = np.float32(1.0)
    gx, gy = (one - fx)[None, :, None], (one - fy)[:, None, None]
    taps = [(np.float32(0.5) * win[r][:, c] / denom).astype(np.float32) for r in (r0, r1) for c in (c0, c1)]
    h0 = taps[0] * gx + taps[1] * fx[None, :, None]
    h1 = taps[2] * gx + taps[3] * fx[None, :, None]
    hdr = (h0 * gy + h1 * fy[:, None, None]).astype(np.float32)
    tap = np.abs(np.maximum(np.maximum(taps[0], taps[1]), np.maximum(taps[2], taps[3])))
    hdr, tap = np.rot90(hdr, k), np.rot90(tap, k)
    if flip0:
        hdr, tap = np.flip(hdr, 0), np.flip(tap, 0)
    if flip1:
        hdr, tap = np.flip(hdr, 1), np.flip(tap, 1)
    return np.ascontiguousarray(hdr), np.ascontiguousarray(tap)
