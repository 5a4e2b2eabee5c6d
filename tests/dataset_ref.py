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
