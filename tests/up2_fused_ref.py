"""Shapes, operands and references of the one-launch low-res form of the up-sampling 3x3 layers (csrc/up2_fused.hip), shared by
tests/test_up2_fused_ref.py (no device) and tests/test_gpu_up2_fused.py.  Pure NumPy.

The kernel restates the two launches of csrc/up2_lowres.hip inside one block, so its model IS conv_ref.up2_lowres followed by
conv_ref.epilogue and conv_ref.project; what this file adds is the list of shapes, the exact operand cases (the recipes of
tests/test_gpu_conv_x3_exact.py), the float64 oracle of the ideal layer, and two deliberately wrong models of the fold."""
import numpy as np

import conv_ref as C
import test_gpu_conv_x3_exact as X                                       # (no device is touched by importing it: the operand recipes live there)
from oracle import ops

TOL = 1e-5                                                               # of the maximum, against the float64 oracle (tests/test_gpu_ops.py)
TOL_PATHS = 5e-6                                                         # of the maximum, between two kernel paths (tests/test_gpu_switches.py)
COUT = 64
TILE_ROWS, TILE_COLS = 6, 14                                             # interior of a block's 8 x 16 low-res patch

# low-res (N, h, w, Cin): every tap clamped; one row; one column; ragged against the 14-wide interior; four chunks ragged both ways; three
# chunks with tiles at the image joins of a batch; several tiles both ways; interior + 1 in each direction
SHAPES = [(2, 1, 1, 64), (1, 1, 7, 64), (1, 6, 1, 64), (1, 5, 33, 64), (1, 17, 15, 128), (3, 9, 29, 96), (2, 13, 31, 128), (1, 7, 15, 64)]


def shape_id(s):
    return "%dx%dx%d_c%d" % s


# (shape, input scale) of the random-operand cases: every shape at scale 1, two of them at 1e-3 and 1e3
RANDOM_CASES = [(s, 1.0) for s in SHAPES] + [(SHAPES[i], k) for i in (3, 5) for k in (1e-3, 1e3)]


# ---------------------------------------------------------------------------------------------------------------------------------
# exact cases: operand mode and epilogue per shape (all four modes; no epilogue, bias, bias + relu, the `up` block's relu - affine - relu)
# ---------------------------------------------------------------------------------------------------------------------------------
def _exact(shape, mode, epi, **o):
    n, h, w, cin = shape
    o.update(name="uf_%s_%s_%s" % (shape_id(shape), mode, epi), n=n, h=h, w=w, cin=cin, cout=COUT, mode=mode, epi=epi)
    if mode != "int":                                                    # thin fine operands: the projected sums of fine outputs stay exact
        o.setdefault("keep", 0.125)
        o.setdefault("kmax", 1)
    return o


EXACT_CASES = [
    _exact(SHAPES[0], "int", "plain"),
    _exact(SHAPES[1], "fx", "relu"),
    _exact(SHAPES[2], "fw", "nobias"),
    _exact(SHAPES[3], "fx", "up"),
    _exact(SHAPES[4], "fxw", "up"),
    _exact(SHAPES[5], "fxw", "relu"),
    _exact(SHAPES[6], "int", "up"),
    _exact(SHAPES[7], "fw", "up"),
]
_REF = {}


def epilogue_of(name, epi, unit, fine):
    """(bias, act1, scale, shift, act2): bias and shift small integers times `unit`, scale a power of two"""
    rng = np.random.default_rng(X.seed_of(name) ^ 0x5EED)
    bias = None if epi == "nobias" else rng.integers(-3, 4, size=COUT) * unit
    act1 = C.ACT_RELU if epi in ("relu", "up") else C.ACT_NONE
    scale = shift = None
    act2 = C.ACT_NONE
    if epi == "up":
        scale = np.ldexp(1.0, rng.integers(-1, 1 if fine else 3, size=COUT))
        shift = rng.integers(-3, 4, size=COUT) * unit
        act2 = C.ACT_RELU
    return bias, act1, scale, shift, act2


def projection_of(name, fine):
    """[3, 64]: small integers; for fine operands two +-1 per row, in the couts of two different waves"""
    rng = np.random.default_rng(X.seed_of(name) ^ 0x9E37)
    if not fine:
        return rng.integers(-2, 3, size=(3, COUT)).astype(np.float64)
    proj = np.zeros((3, COUT))
    for j in range(3):
        g = rng.permutation(4)[:2]
        proj[j, 16 * g + rng.integers(0, 16, size=2)] = rng.choice([-1.0, 1.0], size=2)
    return proj


def exact_reference(o):
    """operands, y and the projected output of an exact case, computed once and left unchanged; asserts that every sum of the GEMM, the
    fold, the epilogue and the projection is exact by construction (below 2^24 units of its terms' lsb), in any order"""
    if o["name"] in _REF:
        return _REF[o["name"]]
    n, h, w, cin, cout = (o[f] for f in ("n", "h", "w", "cin", "cout"))
    fine = o["mode"] != "int"
    x, xb, _, _, wt = X.operands(o["name"], n, h, w, cin, 0, cout, 3, o["mode"], 1.0, o.get("keep", 1.0), o.get("kmax", 2))
    z, v, gemm, stencil = C.up2_lowres(x, xb, wt)
    assert gemm < X.LIMIT, "%s: GEMM sum |terms| / lsb = %.3g 2^24: the accumulator is not exact by construction" % (o["name"], gemm / X.LIMIT)
    assert stencil < X.LIMIT, "%s: stencil A / (lsb_z / 16) = %.3g 2^24: the fold is not exact by construction" % (o["name"], stencil / X.LIMIT)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    # bias and shift on the scale of the layer's output (fine modes: a power of two near max |v| / 4, far above v's lsb)
    unit = 2.0 ** (np.floor(np.log2(np.abs(v).max())) - 2) if fine else 1.0
    bias, act1, scale, shift, act2 = epilogue_of(o["name"], o["epi"], unit, fine)
    vb = v if bias is None else v + bias
    y = C.epilogue(vb, act1, scale, shift, None, act2).astype(np.float64)
    y64 = np.maximum(vb, 0) if act1 else vb                              # the same steps without rounding
    if scale is not None:
        y64 = np.maximum(y64 * scale + shift, 0)
    assert np.array_equal(y, y64), o["name"] + ": the epilogue is not exact by construction"
    proj = projection_of(o["name"], fine)
    yj, tj = C.project(y, proj)
    assert float(tj.max()) / C.common_lsb(y) < X.LIMIT, "%s: projected sums %.3g 2^24: not exact by construction" % (
        o["name"], float(tj.max()) / C.common_lsb(y) / X.LIMIT)
    assert np.array_equal(yj.astype(np.float32).astype(np.float64), yj)
    r = dict(x=x, xb=xb, w=wt, bias=bias, act1=act1, scale=scale, shift=shift, act2=act2, y=y, ymax=float(np.abs(y).max()), proj=proj,
             yj=yj.astype(np.float32))
    for a in (r["y"], r["yj"]):
        a.setflags(write=False)
    _REF[o["name"]] = r
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# random operands: the `up` block (relu, affine, relu) with a projection, against the float64 oracle of the ideal layer
# ---------------------------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def random_operands(shape, xscale=1.0):
    n, h, w, cin = shape
    rng = np.random.default_rng(X.seed_of("uf_random_" + shape_id(shape)))
    x = f32(rng.normal(size=(n, h, w, cin)) * xscale)
    wt = f32(rng.normal(size=(3, 3, cin, COUT)) / np.sqrt(9 * cin))
    return dict(x=x, w=wt, bias=f32(rng.normal(size=COUT) * xscale), scale=f32(rng.uniform(0.5, 1.5, COUT)), shift=f32(rng.normal(size=COUT) * xscale),
                proj=f32(rng.normal(size=(3, COUT))))


def finish(v, o):
    """relu, affine, relu and the projection, in float64"""
    y = np.maximum(np.maximum(v + o["bias"].astype(np.float64), 0) * o["scale"].astype(np.float64) + o["shift"].astype(np.float64), 0)
    return y, y @ o["proj"].astype(np.float64).T


def oracle(o):
    """(y, projected output) of the ideal layer: resize, convolution, epilogue, projection in float64"""
    up = ops.resize_bilinear_2x(o["x"].astype(np.float64))
    return finish(ops.conv2d(up, o["w"].astype(np.float64)), o)


def fold(z, cout, near=0.75, far=0.25, tile_cols=None):
    """conv_ref.up2_lowres_stencil with the two bilinear weights as parameters; tile_cols: the contributions of the low-res column to the
    LEFT of an output's tile of that many columns are dropped (a block that forgets its left halo column)"""
    z = np.asarray(z, dtype=np.float64)
    n, h, w = z.shape[:3]

    def taps(size, t):
        q = np.arange(2 * size) + t - 1
        inside = (q >= 0) & (q < 2 * size)
        qc = np.clip(q, 0, 2 * size - 1)
        m, odd = qc >> 1, (qc & 1) == 1
        return inside, np.where(odd, m, np.maximum(m - 1, 0)), np.where(odd, near, far), np.where(odd, np.minimum(m + 1, size - 1), m), np.where(odd, far, near)

    y = np.zeros((n, 2 * h, 2 * w, cout))
    for ty in range(3):
        rin, *rows = taps(h, ty)
        for tx in range(3):
            sin, *cols = taps(w, tx)
            zt = z[..., (3 * ty + tx) * cout:(3 * ty + tx + 1) * cout]
            inside = (rin[:, None] & sin[None, :])[None, :, :, None]
            for ri, rw in (rows[0:2], rows[2:4]):
                for si, sw in (cols[0:2], cols[2:4]):
                    if tile_cols is not None:
                        sw = np.where(si // tile_cols < (np.arange(2 * w) >> 1) // tile_cols, 0.0, sw)
                    y += np.where(inside, zt[:, ri][:, :, si] * (rw[:, None] * sw[None, :])[None, :, :, None], 0.0)
    return y


def model(o, **wrong):
    """(y, projected output) as the kernel forms them, in float64: the split-operand GEMM at low resolution (conv_ref.up2_lowres), the fold,
    the epilogue; **wrong: the parameters of `fold` that make it a wrong model"""
    z, v, _, _ = C.up2_lowres(o["x"].astype(np.float64), float(np.abs(o["x"]).max()), o["w"].astype(np.float64))
    if wrong:
        v = fold(z, COUT, **wrong)
    return finish(v, o)


def rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))
