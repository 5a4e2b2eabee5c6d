"""Shapes, operands and references of the narrow instantiations of the one-launch low-res form (csrc/up2_fused.hip with 16 or 32 output
channels: the `up` blocks of the Dequantization-Net), for tests/test_gpu_up2_narrow.py.  Pure NumPy.

What tests/up2_fused_ref.py fixes at 64 output channels is restated here with the width as a parameter; its operand modes
(tests/test_gpu_conv_x3_exact.py), its float64 epilogue `finish` and its tolerances are used as they are.  The model of the kernel is
conv_ref.up2_lowres followed by conv_ref.epilogue, whatever the width: a narrow block only maps waves to (patch, 16-cout group)."""
import numpy as np

import conv_ref as C
import test_gpu_conv_x3_exact as X                                       # (no device is touched by importing it: the operand recipes live there)
import up2_fused_ref as U
from oracle import ops

# (Cin, Cout): u1 and u2 of the Dequantization-Net, one chunk into two waves per patch, two chunks into one wave per patch, and the
# 64-cout form at its widest
PAIRS = [(32, 16), (64, 32), (32, 32), (64, 16), (128, 64)]
# low-res (N, h, w) around the 6-row / 14-column interior of a patch; the last two have a patch count that is no multiple of the two or
# four patches of a narrow block (5 and 3 patches), so a block runs with idle waves
GRIDS = [(2, 1, 1), (1, 1, 7), (1, 6, 1), (1, 7, 15), (1, 5, 33), (3, 9, 29), (2, 13, 31), (5, 1, 1), (1, 7, 29)]
EPILOGUES = ("none", "lrelu", "up")                                      # no epilogue; bias + LRELU (the Dequantization-Net); bias + RELU + affine + RELU
MODES = ("int", "fx", "fw", "fxw")


def case_id(pair, grid):
    return "c%dto%d_%dx%dx%d" % (pair + grid)


def exact_cases():
    """every (pair, grid, epilogue); the operand mode goes round the four with the case's number"""
    out = []
    for pair in PAIRS:
        for grid in GRIDS:
            for epi in EPILOGUES:
                mode = MODES[len(out) % len(MODES)]
                o = dict(name="un_%s_%s_%s" % (case_id(pair, grid), mode, epi), n=grid[0], h=grid[1], w=grid[2], cin=pair[0], cout=pair[1],
                         mode=mode, epi=epi)
                if mode != "int":                                        # thin fine operands, as in up2_fused_ref
                    o.update(keep=0.125, kmax=1)
                out.append(o)
    return out


EXACT_CASES = exact_cases()
_REF = {}


def epilogue_of(name, epi, cout, unit, fine):
    """(bias, act1, scale, shift, act2): bias and shift small integers times `unit`, scale a power of two"""
    rng = np.random.default_rng(X.seed_of(name) ^ 0x5EED)
    if epi == "none":
        return None, C.ACT_NONE, None, None, C.ACT_NONE
    bias = rng.integers(-3, 4, size=cout) * unit
    if epi == "lrelu":
        return bias, C.ACT_LRELU, None, None, C.ACT_NONE
    scale = np.ldexp(1.0, rng.integers(-1, 1 if fine else 3, size=cout))
    shift = rng.integers(-3, 4, size=cout) * unit
    return bias, C.ACT_RELU, scale, shift, C.ACT_RELU


def exact_reference(o):
    """operands and y of an exact case, computed once and left unchanged; asserts that every sum of the GEMM and the fold is exact by
    construction (below 2^24 units of its terms' lsb), in any order.  The epilogue is conv_ref.epilogue: fp32 steps rounded once each
    (the LRELU product is the one step that rounds)."""
    if o["name"] in _REF:
        return _REF[o["name"]]
    n, h, w, cin, cout = (o[f] for f in ("n", "h", "w", "cin", "cout"))
    fine = o["mode"] != "int"
    x, xb, _, _, wt = X.operands(o["name"], n, h, w, cin, 0, cout, 3, o["mode"], 1.0, o.get("keep", 1.0), o.get("kmax", 2))
    _, v, gemm, stencil = C.up2_lowres(x, xb, wt)
    assert gemm < X.LIMIT, "%s: GEMM sum |terms| / lsb = %.3g 2^24: the accumulator is not exact by construction" % (o["name"], gemm / X.LIMIT)
    assert stencil < X.LIMIT, "%s: stencil A / (lsb_z / 16) = %.3g 2^24: the fold is not exact by construction" % (o["name"], stencil / X.LIMIT)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    vmax = float(np.abs(v).max())
    unit = 2.0 ** (np.floor(np.log2(vmax)) - 2) if fine and vmax > 0 else 1.0
    bias, act1, scale, shift, act2 = epilogue_of(o["name"], o["epi"], cout, unit, fine)
    vb = v if bias is None else v + bias
    assert np.array_equal(vb.astype(np.float32).astype(np.float64), vb), o["name"] + ": v + bias is not exact by construction"
    y = C.epilogue(vb, act1, scale, shift, None, act2).astype(np.float64)
    r = dict(x=x, xb=xb, w=wt, bias=bias, act1=act1, scale=scale, shift=shift, act2=act2, y=y, ymax=float(np.abs(y).max()))
    y.setflags(write=False)
    _REF[o["name"]] = r
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# random operands
# ---------------------------------------------------------------------------------------------------------------------------------
RANDOM_GRIDS = [(3, 9, 29), (2, 13, 31), (1, 7, 29)]
# (pair, grid, input scale): every pair on the three grids at scale 1, on the first also at 1e-3 and 1e3
RANDOM_CASES = [(p, g, 1.0) for p in PAIRS for g in RANDOM_GRIDS] + [(p, RANDOM_GRIDS[0], k) for p in PAIRS for k in (1e-3, 1e3)]


def random_operands(pair, grid, xscale=1.0):
    cin, cout = pair
    n, h, w = grid
    rng = np.random.default_rng(X.seed_of("un_random_" + case_id(pair, grid)))
    x = U.f32(rng.normal(size=(n, h, w, cin)) * xscale)
    wt = U.f32(rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9 * cin))
    return dict(x=x, w=wt, bias=U.f32(rng.normal(size=cout) * xscale), scale=U.f32(rng.uniform(0.5, 1.5, cout)), shift=U.f32(rng.normal(size=cout) * xscale),
                proj=np.zeros((3, cout), dtype=np.float32))


def oracle(o, epi):
    """y of the ideal layer in float64: resize, convolution, then up2_fused_ref.finish (relu, affine, relu) or bias + LRELU"""
    v = ops.conv2d(ops.resize_bilinear_2x(o["x"].astype(np.float64)), o["w"].astype(np.float64))
    if epi == "up":
        return U.finish(v, o)[0]
    vb = v + o["bias"].astype(np.float64)
    return np.where(vb >= 0, vb, vb * float(C.LRELU_SLOPE))
