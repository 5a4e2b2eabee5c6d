"""NumPy restatement of the HDR-Real folder reader (singlehdr-tf2_amd/hdr_real.py, csrc/hdr_real.hip) for the tests: the patch
filter of convert_to_tf_record.py:54-56, the normalisation and augmentation of finetune_real_dataset.py:47-60.  Float64 where
the product sums in float64; np.fliplr / np.rot90 for the augmentation; every fp32 step is one rounded NumPy float32 operation."""
import numpy as np

F = np.float32
CR, CG, CB = F(0.299), F(0.587), F(0.114)
GRAY_HI, GRAY_LO = F(249.0), F(6.0)


def gray(r, g, b):
    """the specified order: fp32, left to right, unfused -- (r*0.299f + g*0.587f) + b*0.114f, five roundings"""
    r, g, b = (np.asarray(v).astype(F) for v in (r, g, b))
    return (r * CR + g * CG) + b * CB


def gray_fused(r, g, b):
    """the same expression with every multiply-add contracted: fma(b, 0.114f, fma(g, 0.587f, r*0.299f)).  In float64 the
    product of two fp32 values and its sum with a third of this magnitude are exact, so one rounding to fp32 per fma"""
    r, g, b = (np.asarray(v).astype(np.float64) for v in (r, g, b))
    t = (r * np.float64(CR)).astype(F)
    t = (g * np.float64(CG) + t.astype(np.float64)).astype(F)
    return (b * np.float64(CB) + t.astype(np.float64)).astype(F)


def gray_reversed(r, g, b):
    """unfused fp32, right to left: (b*0.114f + g*0.587f) + r*0.299f"""
    r, g, b = (np.asarray(v).astype(F) for v in (r, g, b))
    return (b * CB + g * CG) + r * CR


def extreme(gr):
    return (gr >= GRAY_HI) | (gr <= GRAY_LO)


def patch_stats(ldr_patch, hdr_patch):
    """(extreme-pixel count, float32 mean of the float64 sum) of one patch pair"""
    count = int(extreme(gray(ldr_patch[..., 0], ldr_patch[..., 1], ldr_patch[..., 2])).sum())
    h = np.asarray(hdr_patch, dtype=F)
    return count, F(np.sum(h.astype(np.float64)) / np.float64(h.size))


def augment(patch, flip, rot):
    """tf.image.rot90(flip_left_right(x) if flip else x, k): counter-clockwise, k = 4 is a full turn"""
    return np.rot90(np.fliplr(patch) if flip else patch, int(rot) % 4)


def render(ldr_patch, hdr_patch, mean, flip, rot):
    """(ref_LDR, ref_HDR) of one sample: one fp32 division; one fp32 division then one fp32 multiplication, with the STORED mean"""
    ldr = augment(np.asarray(ldr_patch).astype(F), flip, rot) / F(255.0)
    hdr = augment(np.asarray(hdr_patch, dtype=F), flip, rot) / (F(1e-6) + F(mean)) * F(0.5)
    return np.ascontiguousarray(ldr, dtype=F), np.ascontiguousarray(hdr, dtype=F)


def crop(img, h1, w1, size):
    return img[h1:h1 + size, w1:w1 + size]
