"""The deterministic entry points (include/shdr.h "Deterministic mode"), one by one, through the C ABI.

Per launch site:
  * exact -- on the integer operands of tests/test_gpu_wgrad_f32_exact.py (every sum is exact in any order) the deterministic result, the
    default-path result and the float64 reference are the same BIT PATTERNS over the whole tensor, into zeros and into integers, with the
    -12345 / -0.0 sentinels in the elements the call does not own and guard words around the tensor;
  * order-sensitive -- on operands of mixed magnitude (normal values times 2^k, k uniform in [-10, 10] per element) five runs are
    bit-identical, and the result is within the existing op-level bar of float64 (1e-4 of the tensor's scale for gradients, 2e-4 for the
    CRF head, tape_ref.sum_bar / the existing per-op bars for sums), no element exempt;
  * accumulate identity -- det(out = g0.clone()) is exactly g0 + det(out = zeros);
  * the counter -- shdr_order_dependent_launches() does not move in a deterministic call and moves in the default one.
Every case asserts from the workspace query that it has at least two slabs / partial rows: with one, nothing is folded.

Shapes are those of tests/test_gpu_wgrad_f32_exact.py and tests/test_gpu_tape_f32.py for the family, enlarged only to get a second slab.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as C
import tape_ref as F
import test_gpu_tape_f32 as E
import test_gpu_wgrad_f32_exact as W
from conftest import rel_err

pytestmark = pytest.mark.gpu

S8 = W.S8
RUNS = 5
(DET_WGRAD, DET_BIAS_GRAD, DET_ACT_BWD_BIAS, DET_BATCHNORM, DET_DIFF_LOSS, DET_TV_LOSS, DET_SAMPLE_DOT, DET_INVCRF, DET_APPLY_RF, DET_WINOGRAD,
 DET_X3) = range(11)
GRAD_BAR = 1e-4                                 # the op-level bar of a gradient tensor: max |err| / max |reference|
CRF_BAR = 2e-4                                  # ... of the CRF head
FWD_BAR = 1e-5                                  # ... of a forward value


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


P = W.P


def ws_of(lib, op, d=None, n=0, c=0, k=0):
    nbytes = lib.shdr_det_workspace_bytes(op, None if d is None else ctypes.byref(d), n, c, k)
    assert nbytes > 0, (op, n, c, k, nbytes)
    # poisoned: the entry points must not need a zeroed workspace
    return torch.full((nbytes // 4 + 4,), float("nan"), device="cuda", dtype=torch.float32), nbytes


def mixed(rng, shape):
    """normal values times 2^k, k uniform in [-10, 10] per element"""
    return (rng.normal(size=shape) * np.exp2(rng.integers(-10, 11, size=shape))).astype(np.float32)


def counter(lib):
    return lib.shdr_order_dependent_launches()


def bits(t):
    torch.cuda.synchronize()
    return t.detach().clone().view(torch.int32)


def five_equal(run, what):
    """run() -> tensor or tuple of tensors; five runs, bit-identical; returns the first"""
    first = run()
    first = first if isinstance(first, tuple) else (first,)
    ref = [bits(t) for t in first]
    for i in range(1, RUNS):
        got = run()
        got = got if isinstance(got, tuple) else (got,)
        for j, (a, b) in enumerate(zip(ref, got)):
            assert torch.equal(a, bits(b)), "%s: run %d differs from run 0 in output %d (%d elements)" % (what, i, j, int((a != bits(b)).sum()))
    return first


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_conv2d_wgrad_det_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def wgrad_det(K, lib, d, src, which, dz, dw):
    ws, nws = ws_of(lib, DET_WGRAD, d, c=which)
    before = counter(lib)
    rc = lib.shdr_conv2d_wgrad_det_f32(ctypes.byref(d), P(src), which, P(dz), P(dw), P(ws), nws, K._stream())
    assert rc == 0, (rc, lib.shdr_last_error())
    assert counter(lib) == before, "the deterministic weight gradient moved the counter"
    return ws


def slabs(lib, d, which, k, ct, cols):
    nbytes = lib.shdr_det_workspace_bytes(DET_WGRAD, ctypes.byref(d), 0, which, 0)
    slab = k * k * ct * cols * 4
    assert nbytes > 0 and nbytes % slab == 0, (nbytes, slab)
    return nbytes // slab


def run_wgrad_exact(K, lib, case, monkeypatch):
    """W.run_wgrad with the deterministic call beside the default one: both equal the reference bit for bit"""
    name, n, h, w, c1, c2, cz, k, stride, x2s, tile, o = case
    if o.get("env"):
        monkeypatch.setenv(o["env"], "1")
    x, x2, dz = W.operands(len(name) * 41 + h * 3 + w, n, h, w, c1, c2, cz, k, stride, x2s)
    ref = C.wgrad(x, x2, dz, (k, k, c1 + c2, cz), stride, x2s, None)
    npix = dz.shape[0] * dz.shape[1] * dz.shape[2]
    moved = 0
    for accumulate in (False, True):
        base = W.base_of(ref.shape, accumulate, c1 * 7 + cz)
        W.precondition([(x, 1.0)] + ([(x2, x2s)] if c2 else []), dz, npix, base, name)
        buf, v = W.guarded(ref.size)
        dw = v.view(torch.float32).view(ref.shape)
        d = W.desc_of(K, x.shape, c2, k, cz, stride, x2s, o.get("cout"), o.get("algo", W.AUTO))
        dzd = W.f32(dz)
        for which, src, r0, r1 in ((0, x, 0, c1),) + (((1, x2, c1, c1 + c2),) if c2 else ()):
            assert slabs(lib, d, which, k, c1 + c2, cz) >= 2, "%s: one slab only, nothing would be folded" % name
            init = W.forbidden(ref.shape)
            init[:, :, r0:r1] = base[:, :, r0:r1]
            want = init.copy()
            want[:, :, r0:r1] += ref[:, :, r0:r1].astype(np.float32)
            xd = W.f32(src)
            dw.copy_(torch.from_numpy(init))
            wgrad_det(K, lib, d, xd, which, dzd, dw)
            W.guards_intact(buf, ref.size, name)
            W.same(dw.cpu().numpy(), want, "%s, deterministic (source %d, accumulate %d)" % (name, which, accumulate), tile)
            dw.copy_(torch.from_numpy(init))
            before = counter(lib)
            assert lib.shdr_conv2d_wgrad_f32(ctypes.byref(d), P(xd), which, P(dzd), P(dw), K._stream()) == 0
            moved += counter(lib) - before
            W.same(dw.cpu().numpy(), want, "%s, default (source %d, accumulate %d)" % (name, which, accumulate), tile)
    return moved


# id, n, h, w, c1, c2, cols, k, stride, x2s, (BMc, BNc), opts -- the tuple of W.MFMA_CASES.  2115 pixels: three slices of 1024 (32 x 33)
MFMA_DET = [("tile_%dx%d_2115" % (bm, bn), 1, 47, 45, cx, 0, cz, 3, 1, 1.0, (bm, bn), {})
            for cx, cz, bm, bn in ((16, 16, 16, 16), (32, 32, 32, 32), (64, 64, 64, 64), (96, 64, 96, 64), (128, 128, 128, 128), (16, 128, 16, 128),
                                   (128, 16, 128, 16), (96, 16, 32, 16), (64, 32, 64, 32))]
MFMA_DET += [
    ("ragged_cols48_three_16_tiles", 1, 47, 45, 32, 0, 48, 3, 1, 1.0, (32, 16), {}),
    ("ragged_cx48_three_16_tiles", 1, 47, 45, 48, 0, 32, 3, 1, 1.0, (16, 32), {}),
    ("ragged_two_sources_32_32_scaled", 1, 47, 45, 32, 32, 64, 3, 1, S8, (32, 64), {}),
    ("ragged_two_sources_64_16_half_k1", 1, 47, 45, 64, 16, 16, 1, 1, 0.5, (64, 16), {}),
    ("ragged_s2_7x7_stem_96_64", 2, 47, 45, 96, 0, 64, 7, 2, 1.0, (96, 64), {}),                  # 2 x 24 x 23 = 1104 output pixels
    ("ragged_s2_3x3_odd", 2, 47, 45, 32, 0, 64, 3, 2, 1.0, (32, 64), {}),
    ("cout_valid_16_of_32_two_sources", 1, 47, 45, 16, 16, 16, 3, 1, S8, (16, 16), {"cout": 32}),
    ("k5_32_64", 1, 47, 45, 32, 0, 64, 5, 1, 1.0, (32, 64), {}),
    ("no_wgrad96_cx96_on_32_tiles", 1, 47, 45, 96, 0, 64, 3, 1, 1.0, (32, 64), {"env": "SHDR_NO_WGRAD96"}),
]


@pytest.mark.parametrize("case", MFMA_DET, ids=[c[0] for c in MFMA_DET])
def test_wgrad_mfma_exact(K, lib, case, monkeypatch):
    monkeypatch.setenv("SHDR_NO_ALLTAPS", "1")
    assert run_wgrad_exact(K, lib, case, monkeypatch) > 0                            # the default form counts


# the eight instantiations of wgrad_alltaps_kernel; 1 x 33 x 50: 66 row segments, one slab each
ALLTAPS_DET = [("alltaps_k%d_%d_%d" % (k, cx, cz), 1, 33, 50, cx, 0, cz, k, 1, 1.0, (cx, cz), {})
               for k, cx, cz in ((3, 16, 16), (3, 16, 32), (3, 32, 16), (3, 32, 32), (5, 16, 16), (5, 16, 32), (5, 32, 16), (7, 16, 16))]
ALLTAPS_DET += [
    ("alltaps_two_sources_32_32_scaled", 1, 33, 50, 32, 32, 32, 3, 1, S8, (32, 32), {}),
    ("alltaps_two_sources_16_32_half_k5", 1, 5, 70, 16, 32, 16, 5, 1, 0.5, (16, 16), {}),
    ("alltaps_two_units_per_block_k3_32_16", 1, 70, 150, 32, 0, 16, 3, 1, 1.0, (32, 16), {}),    # 350 segments on 256 blocks: 2 per block
]


@pytest.mark.parametrize("case", ALLTAPS_DET, ids=[c[0] for c in ALLTAPS_DET])
def test_wgrad_all_taps_exact(K, lib, case, monkeypatch):
    assert run_wgrad_exact(K, lib, case, monkeypatch) > 0


DIRECT_DET = [
    ("direct_4_16_pixels_1025", 1, 25, 41, 4, 0, 16, 3, 1, 1.0, (4, 16), {}),
    ("direct_two_sources_3_4_scaled", 1, 25, 41, 3, 4, 3, 3, 1, S8, (3, 3), {}),
    ("direct_16_3_of_16_pixels_2049", 1, 3, 683, 16, 0, 3, 3, 1, 1.0, (16, 3), {"cout": 16}),
    ("direct_algo_on_32_32", 1, 25, 41, 32, 0, 32, 3, 1, 1.0, (32, 32), {"algo": W.DIRECT}),
]


@pytest.mark.parametrize("case", DIRECT_DET, ids=[c[0] for c in DIRECT_DET])
def test_wgrad_direct_exact(K, lib, case, monkeypatch):
    assert run_wgrad_exact(K, lib, case, monkeypatch) > 0


# ---- the Winograd-domain and split-operand families: the exact tests of tests/test_gpu_wgrad_f32_exact.py, run on the slab forms ---------
class DetLib:
    """the library with shdr_conv2d_wgrad_winograd_f32 and shdr_conv2d_wgrad_x3_f32 answered by their deterministic forms (a poisoned
    workspace per call; at least two slabs, from the query; the counter stands still)"""

    def __init__(self, K, lib):
        self._K, self._lib, self.calls = K, lib, 0

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def shdr_conv2d_wgrad_winograd_f32(self, x, dz, du, dw, n, h, w, cx, cout, ct, off, s, stream):
        d = self._K._conv_desc((n, h, w, cx), (3, 3, cx, cout), 1, 0, 1.0, None)
        ws, nws = ws_of(self._lib, DET_WINOGRAD, d, c=0)
        assert nws % (16 * cx * cout * 4) == 0 and nws // (16 * cx * cout * 4) >= 2, "one slab only"
        before = counter(self._lib)
        rc = self._lib.shdr_conv2d_wgrad_winograd_det_f32(x, dz, du, dw, P(ws), nws, n, h, w, cx, cout, ct, off, s, stream)
        torch.cuda.synchronize()
        assert counter(self._lib) == before
        self.calls += 1
        return rc

    def shdr_conv2d_wgrad_x3_f32(self, d, xh, xl, which, zh, zl, xr, zr, dw, stream):
        desc = d._obj
        ws, nws = ws_of(self._lib, DET_X3, desc, c=which)
        slab = desc.KH * desc.KW * (desc.C1 + desc.C2) * desc.Cout * 4
        assert nws % slab == 0 and nws // slab >= 2, "one slab only"
        before = counter(self._lib)
        rc = self._lib.shdr_conv2d_wgrad_x3_det_f32(d, xh, xl, which, zh, zl, xr, zr, dw, P(ws), nws, stream)
        torch.cuda.synchronize()
        assert counter(self._lib) == before
        self.calls += 1
        return rc


WINO_DET = [c for c in W.WINO if c[0] in ("wino_32_64_slices_3x33x50", "wino_64_192_1x33x50", "wino_96_128_3x33x50",
                                          "wino_two_sources_64_32_scaled_slices", "wino_accumulate", "wino_accumulate_two_sources_half")]
X3_DET = [c for c in W.X3_CASES if c[0] in ("x3_64x64_cx64_cz64_pixels_1650", "x3_128x128_cx128_cz128_pixels_1650_slices",
                                            "x3_two_sources_64_128_scaled_1650", "x3_accumulate_64_64_slices")]
assert len(WINO_DET) == 6 and len(X3_DET) == 4


@pytest.mark.parametrize("case", WINO_DET, ids=[c[0] for c in WINO_DET])
def test_wgrad_winograd_exact(K, lib, case):
    """whole-tensor bit patterns against the float64 reference, sentinels in the other source's rows, guards around dw and the dU scratch"""
    name, n, h, w, c1, c2, cout, x2s, acc = case
    det = DetLib(K, lib)
    W.run_winograd(K, det, n, h, w, c1, c2, cout, x2s, acc, name, len(name) * 13 + h)
    assert det.calls == (2 if c2 else 1)
    before = counter(lib)
    W.run_winograd(K, lib, n, h, w, c1, c2, cout, x2s, acc, name, len(name) * 13 + h)          # the default form: the same bits, and it counts
    assert counter(lib) > before


@pytest.mark.parametrize("fine", ["x", "dz"])
@pytest.mark.parametrize("case", X3_DET, ids=[c[0] for c in X3_DET])
def test_wgrad_split_operand_exact(K, lib, case, fine):
    det = DetLib(K, lib)
    W.test_split_operand_kernel(K, det, case, fine)
    assert det.calls == (2 if case[5] else 1)
    before = counter(lib)
    W.test_split_operand_kernel(K, lib, case, fine)
    assert counter(lib) > before


ORDER_CASES = [("mfma_32_64_two_sources", 1, 47, 45, 32, 32, 64, 3, 1, S8, "SHDR_NO_ALLTAPS"),
               ("mfma_stem_s2_7x7_96_64", 2, 47, 45, 96, 0, 64, 7, 2, 1.0, None),
               ("alltaps_k3_32_32_two_sources", 1, 33, 50, 32, 32, 32, 3, 1, S8, None),
               ("alltaps_k7_16_16", 1, 33, 50, 16, 0, 16, 7, 1, 1.0, None),
               ("direct_4_16", 1, 25, 41, 4, 0, 16, 3, 1, 1.0, None)]


@pytest.mark.parametrize("case", ORDER_CASES, ids=[c[0] for c in ORDER_CASES])
def test_wgrad_order_sensitive_and_accumulate_identity(K, lib, case, monkeypatch):
    name, n, h, w, c1, c2, cz, k, stride, x2s, env = case
    if env:
        monkeypatch.setenv(env, "1")
    rng = np.random.default_rng(len(name) + h)
    x, dz = mixed(rng, (n, h, w, c1)), mixed(rng, (n, -(-h // stride), -(-w // stride), cz))
    x2 = mixed(rng, (n, h, w, c2)) if c2 else None
    ref = C.wgrad(x, x2, dz, (k, k, c1 + c2, cz), stride, x2s, None)
    d = W.desc_of(K, x.shape, c2, k, cz, stride, x2s)
    xd, x2d, dzd = E.fd(x), (E.fd(x2) if c2 else None), E.fd(dz)
    g0 = E.fd(mixed(rng, ref.shape))

    def run(into):
        dw = into.clone()
        for which, src in ((0, xd),) + (((1, x2d),) if c2 else ()):
            assert slabs(lib, d, which, k, c1 + c2, cz) >= 2
            wgrad_det(K, lib, d, src, which, dzd, dw)
        return dw
    (dw,) = five_equal(lambda: run(torch.zeros_like(g0)), name)
    err = rel_err(E.back(dw), ref)
    print("%s: %.3e of the float64 reference (bar %.0e)" % (name, err, GRAD_BAR))
    assert err <= GRAD_BAR
    assert torch.equal(run(g0), g0 + dw), name + ": accumulating into g0 is not g0 + (the result into zeros)"


# ---------------------------------------------------------------------------------------------------------------------------------
# bias gradients: shdr_bias_grad_det_f32, shdr_act_bwd_bias_det_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def rows_of(lib, op, n, c, row_bytes, k=0):
    nbytes = lib.shdr_det_workspace_bytes(op, None, n, c, k)
    assert nbytes > 0 and nbytes % row_bytes == 0, (op, nbytes, row_bytes)
    return nbytes // row_bytes


def guarded_f32(init):
    buf, v = W.guarded(init.size)
    out = v.view(torch.float32).view(init.shape)
    out.copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)))
    return buf, out


@pytest.mark.parametrize("npix,c", [(2115, 16), (5000, 3), (2115, 48), (700, 300)], ids=str)
def test_bias_grad(K, lib, npix, c):
    rng = np.random.default_rng(npix + c)
    assert rows_of(lib, DET_BIAS_GRAD, npix, c, 4 * c) >= 2
    dz = E.ints(rng, (npix, c), -4, 4)
    dzd = E.fd(dz)
    want = dz.astype(np.float64).sum(axis=0)
    for base in (np.zeros(c), rng.integers(-50, 51, size=c)):
        ws, nws = ws_of(lib, DET_BIAS_GRAD, n=npix, c=c)
        buf, db = guarded_f32(base)
        before = counter(lib)
        E.call(lib, K, "shdr_bias_grad_det_f32", P(dzd), P(db), P(ws), nws, npix, c)
        assert counter(lib) == before
        W.guards_intact(buf, c, "bias_grad_det")
        W.same(E.back(db), (base + want).astype(np.float32), "bias_grad_det")
        buf, db = guarded_f32(base)
        E.call(lib, K, "shdr_bias_grad_f32", P(dzd), P(db), npix, c)
        assert counter(lib) == before + 1
        W.same(E.back(db), (base + want).astype(np.float32), "bias_grad default")
    m = mixed(rng, (npix, c))
    md, g0 = E.fd(m), E.fd(mixed(rng, c))

    def run(into):
        db = into.clone()
        ws, nws = ws_of(lib, DET_BIAS_GRAD, n=npix, c=c)
        E.call(lib, K, "shdr_bias_grad_det_f32", P(md), P(db), P(ws), nws, npix, c)
        return db
    (db,) = five_equal(lambda: run(torch.zeros_like(g0)), "bias_grad_det")
    E.assert_bar(E.back(db), m.astype(np.float64).sum(axis=0), F.sum_bar(m, axis=0, extra=2), "bias_grad_det")
    assert torch.equal(run(g0), g0 + db)


ACT_CASES = [(2115, 64, F.ACT_RELU, "133 rows"), (1027, 16, F.ACT_NONE, "17 rows, no activation"), (700, 1024, F.ACT_LRELU, "Q = 256"),
             (16384, 1024, F.ACT_RELU, "nquads = 2^22: 2048 rows, where the default fold ends in atomics over eight row slices")]


@pytest.mark.parametrize("case", ACT_CASES, ids=[c[3] for c in ACT_CASES])
def test_act_bwd_bias(K, lib, case):
    npix, c, act, _ = case
    rng = np.random.default_rng(npix + c)
    rows = rows_of(lib, DET_ACT_BWD_BIAS, npix, c, 4 * c)
    assert rows >= 2 and rows * 4 * c <= lib.shdr_workspace_bytes(4, None, c)
    dy, y = E.ints(rng, (npix, c), -4, 4), E.ints(rng, (npix, c), -2, 2)
    if act == F.ACT_LRELU:                              # 0.1 g is not exact: the exact part stays on the positive side (slope 1)
        y = np.abs(y) + 1
    dyd, yd = E.fd(dy), E.fd(y)
    dzr = dy.astype(np.float64) * (1.0 if act == F.ACT_NONE else (y > 0) * 1.0)
    want = dzr.sum(axis=0)
    assert np.abs(dzr).sum(axis=0).max() < 2 ** 24
    for base in (np.zeros(c), rng.integers(-50, 51, size=c)):
        for fn, moves in (("shdr_act_bwd_bias_det_f32", 0), ("shdr_act_bwd_bias_f32", 1 if rows > 256 else 0)):
            ws = torch.full((rows * c,), float("nan"), device="cuda")
            buf, db = guarded_f32(base)
            dz = torch.empty_like(dyd)
            before = counter(lib)
            E.call(lib, K, fn, P(dyd), P(yd) if act else None, P(dz) if act else None, P(db), P(ws), npix, c, act)
            assert counter(lib) == before + moves, fn
            W.guards_intact(buf, c, fn)
            W.same(E.back(db), (base + want).astype(np.float32), fn)
            if act:
                E.assert_equal(E.back(dz), dzr, fn + " dz")
    m, my = mixed(rng, (npix, c)), E.f32(rng, (npix, c))
    md, myd, g0 = E.fd(m), E.fd(my), E.fd(mixed(rng, c))

    def run(into):
        db, dz = into.clone(), torch.empty_like(md)
        ws = torch.full((rows * c,), float("nan"), device="cuda")
        E.call(lib, K, "shdr_act_bwd_bias_det_f32", P(md), P(myd) if act else None, P(dz) if act else None, P(db), P(ws), npix, c, act)
        return db
    (db,) = five_equal(lambda: run(torch.zeros_like(g0)), "act_bwd_bias_det")
    terms = m.astype(np.float64) * {F.ACT_NONE: 1.0, F.ACT_RELU: (my > 0) * 1.0, F.ACT_LRELU: np.where(my > 0, 1.0, float(np.float32(0.1)))}[act]
    E.assert_bar(E.back(db), terms.sum(axis=0), F.sum_bar(terms, axis=0, extra=3), "act_bwd_bias_det")
    assert torch.equal(run(g0), g0 + db)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm with C % 4 != 0: the scalar reduction
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix,c", [(5000, 6), (9000, 3)], ids=str)
def test_batchnorm_scalar_reduction(K, lib, npix, c):
    rng = np.random.default_rng(npix + c)
    rows = rows_of(lib, DET_BATCHNORM, npix, c, 16 * c) - 1
    assert rows >= 2 and (rows + 1) * 16 * c <= lib.shdr_workspace_bytes(3, None, c)
    eps = 1e-3
    x, dy = mixed(rng, (npix, c)), mixed(rng, (npix, c))
    gamma = E.f32(rng, c)
    xd, dyd, gd = E.fd(x), E.fd(dy), E.fd(gamma)
    nws = lib.shdr_workspace_bytes(3, None, c)

    def stats(fn):
        ws = torch.full((nws // 8,), float("nan"), device="cuda", dtype=torch.float64)
        mean, var = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
        E.call(lib, K, fn, P(xd), P(ws), P(mean), P(var), None, None, npix, c, 0.99)
        return mean, var
    before = counter(lib)
    mean, var = five_equal(lambda: stats("shdr_bn_stats_det_f32"), "bn_stats_det")
    assert counter(lib) == before
    x64 = x.astype(np.float64)
    assert rel_err(E.back(mean), x64.mean(axis=0)) <= 1e-5 and rel_err(E.back(var), x64.var(axis=0)) <= 1e-5          # the forward bar
    stats("shdr_bn_stats_f32")
    assert counter(lib) == before + 1
    g0g, g0b = E.fd(mixed(rng, c)), E.fd(mixed(rng, c))

    def bwd(into_g, into_b):
        ws = torch.full((nws // 8,), float("nan"), device="cuda", dtype=torch.float64)
        dgamma, dbeta, dx = into_g.clone(), into_b.clone(), torch.empty_like(xd)
        E.call(lib, K, "shdr_bn_bwd_ranged_det_f32", P(dyd), P(xd), None, P(mean), P(var), P(gd), P(ws), P(dgamma), P(dbeta), P(dx), npix, c, eps,
               None)
        return dgamma, dbeta, dx
    before = counter(lib)
    dgamma, dbeta, dx = five_equal(lambda: bwd(torch.zeros_like(g0g), torch.zeros_like(g0b)), "bn_bwd_det")
    assert counter(lib) == before
    mu, va = E.back(mean).astype(np.float64), E.back(var).astype(np.float64)
    inv = 1.0 / np.sqrt(va + eps)
    g64 = dy.astype(np.float64)
    xh = (x64 - mu) * inv
    rb, rg = g64.sum(axis=0), (g64 * xh).sum(axis=0)
    rdx = gamma * inv * (g64 - rb / npix - xh * rg / npix)
    for got, ref, what in ((dgamma, rg, "dgamma"), (dbeta, rb, "dbeta"), (dx, rdx, "dx")):
        err = rel_err(E.back(got), ref)
        print("bn_bwd_det %s: %.3e" % (what, err))
        assert err <= GRAD_BAR, what
    a, b, _ = bwd(g0g, g0b)
    assert torch.equal(a, g0g + dgamma) and torch.equal(b, g0b + dbeta)


# ---------------------------------------------------------------------------------------------------------------------------------
# the CRF head: shdr_invcrf_decode_bwd_det_f32, shdr_apply_rf_bwd_det_f32
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,f", [(3, 255), (2, 512), (3, 1)], ids=str)
def test_invcrf_decode_bwd(K, lib, b, f):
    rng = np.random.default_rng(b * 7 + f)
    k = 1024
    assert rows_of(lib, DET_INVCRF, 0, b, (f + 1) * 11 * 4, f) == b >= 2
    table, wfc, feat, dinv = E.ints(rng, (k, 12), -3, 3), E.ints(rng, (f, 11), -2, 2), E.ints(rng, (b, f), -3, 3), E.ints(rng, (b, k), -3, 3)
    rf_, rw, rb = F.invcrf_decode_bwd(dinv, feat, wfc, table)
    assert np.abs(rw).max() < 2 ** 24

    def run(fn, args, into_w, into_b):
        dinv_, feat_, wfc_, table_ = args
        dfeat, dwfc, dbfc = torch.empty_like(feat_), into_w.clone(), into_b.clone()
        if fn.endswith("det_f32"):
            ws, nws = ws_of(lib, DET_INVCRF, c=b, k=f)
            E.call(lib, K, fn, P(dinv_), P(feat_), P(wfc_), P(table_), P(dfeat), P(dwfc), P(dbfc), P(ws), nws, b, f, k)
        else:
            E.call(lib, K, fn, P(dinv_), P(feat_), P(wfc_), P(table_), P(dfeat), P(dwfc), P(dbfc), b, f, k)
        return dfeat, dwfc, dbfc
    args = tuple(E.fd(t) for t in (dinv, feat, wfc, table))
    for base_w, base_b in ((np.zeros((f, 11)), np.zeros(11)), (rng.integers(-50, 51, size=(f, 11)), rng.integers(-50, 51, size=11))):
        for fn, moves in (("shdr_invcrf_decode_bwd_det_f32", 0), ("shdr_invcrf_decode_bwd_f32", 1)):
            before = counter(lib)
            dfeat, dwfc, dbfc = run(fn, args, E.fd(base_w), E.fd(base_b))
            assert counter(lib) == before + moves
            E.assert_equal(E.back(dfeat), rf_, fn)
            W.same(E.back(dwfc), (base_w + rw).astype(np.float32), fn + " dwfc")
            W.same(E.back(dbfc), (base_b + rb).astype(np.float32), fn + " dbfc")
    table, wfc, feat, dinv = mixed(rng, (k, 12)), E.f32(rng, (f, 11)), mixed(rng, (b, f)), mixed(rng, (b, k))
    args = tuple(E.fd(t) for t in (dinv, feat, wfc, table))
    g0w, g0b = E.fd(mixed(rng, (f, 11))), E.fd(mixed(rng, 11))
    dfeat, dwfc, dbfc = five_equal(lambda: run("shdr_invcrf_decode_bwd_det_f32", args, torch.zeros_like(g0w), torch.zeros_like(g0b)), "invcrf det")
    for got, ref, what in zip((dfeat, dwfc, dbfc), F.invcrf_decode_bwd(dinv, feat, wfc, table), ("dfeat", "dwfc", "dbfc")):
        err = rel_err(E.back(got), ref)
        print("invcrf_decode_bwd_det %s: %.3e" % (what, err))
        assert err <= CRF_BAR, what
    _, a, bb = run("shdr_invcrf_decode_bwd_det_f32", args, g0w, g0b)
    assert torch.equal(a, g0w + dwfc) and torch.equal(bb, g0b + dbfc)


@pytest.mark.parametrize("K_", [2, 1024, 4096])
@pytest.mark.parametrize("npb", [1027, 70001], ids=str)           # 70 001 > 256 blocks x 256: a second trip of the staged loop
def test_apply_rf_bwd(K, lib, K_, npb):
    """test_gpu_tape_f32.py::test_apply_rf_bwd on the deterministic entry point"""
    rng = np.random.default_rng(K_ * 3 + npb)
    nb = 2
    slabs_ = rows_of(lib, DET_APPLY_RF, npb, nb, nb * K_ * 4, K_)
    assert slabs_ == min(-(-npb // 256), 256) >= 2
    rf = np.sort(rng.random((nb, K_)), axis=1).astype(np.float32)
    rfd = E.fd(rf)

    def run(xd, dyd, need_dx, into):
        drf = into.clone()
        dx = torch.empty_like(xd) if need_dx else None
        ws, nws = ws_of(lib, DET_APPLY_RF, n=npb, c=nb, k=K_)
        before = counter(lib)
        E.call(lib, K, "shdr_apply_rf_bwd_det_f32", P(xd), P(rfd), P(dyd), P(drf), P(dx), P(ws), nws, nb, npb, K_)
        assert counter(lib) == before
        return (drf, dx) if need_dx else drf
    zeros = torch.zeros((nb, K_), device="cuda")
    # (1) x on exact knots, integer dy: drf[k] is the integer sum of the gradients that hit knot k
    kx, kk = E.knot_x(K_, rng, nb * npb)
    x, dy = kx.reshape(nb, npb), E.ints(rng, (nb, npb), -8, 8)
    want = np.zeros((nb, K_))
    np.add.at(want, (np.repeat(np.arange(nb), npb), kk), dy.reshape(-1))
    base = rng.integers(-50, 51, size=(nb, K_)).astype(np.float32)
    E.assert_equal(E.back(run(E.fd(x), E.fd(dy), False, zeros)), want, "drf on knots")
    E.assert_equal(E.back(run(E.fd(x), E.fd(dy), False, E.fd(base))), base + want, "drf on knots, accumulated")
    # (2) x strictly inside the intervals, gradients of mixed magnitude
    k0 = rng.integers(0, K_ - 1, size=(nb, npb))
    x = ((k0 + rng.uniform(0.05, 0.95, size=(nb, npb))) / (K_ - 1)).astype(np.float32)
    dy = mixed(rng, (nb, npb))
    xd, dyd = E.fd(x), E.fd(dy)
    drf, dx = five_equal(lambda: run(xd, dyd, True, zeros), "apply_rf_bwd_det")
    rdrf, rdx = F.apply_rf_bwd(x, rf, dy)
    adrf, adx = F.apply_rf_bwd(x, rf, dy, absolute=True)
    E.assert_bar(E.back(dx), rdx, F.bar32(3, adx), "dx")
    yv, i0, i1, w0, w1 = F.apply_rf_parts(x, K_)
    g = np.abs(dy.astype(np.float64))
    acc, cnt = np.zeros((nb, K_)), np.zeros((nb, K_))
    rows = np.broadcast_to(np.arange(nb)[:, None], i0.shape)
    for idx, wt in ((i0, w0), (i1, w1)):
        np.add.at(acc, (rows, idx), g * (yv + wt))
        np.add.at(cnt, (rows, idx), 1.0)
    E.assert_bar(E.back(drf), rdrf, F.U32 * acc + (cnt + 1) * F.U32 * adrf, "drf")       # the bar of the default kernel's test
    g0 = E.fd(mixed(rng, (nb, K_)))
    assert torch.equal(run(xd, dyd, False, g0), g0 + drf)
    before = counter(lib)
    E.call(lib, K, "shdr_apply_rf_bwd_f32", P(xd), P(rfd), P(dyd), P(zeros.clone()), None, nb, npb, K_)
    assert counter(lib) == before + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# forward sums
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("npb", [257, 33000])
def test_diff_loss_and_sample_dot(K, lib, nb, npb):
    rng = np.random.default_rng(nb + npb)
    blocks = rows_of(lib, DET_DIFF_LOSS, npb, nb, 4 * nb)
    assert blocks == min(-(-npb // 256), 128) >= 2 and blocks == rows_of(lib, DET_SAMPLE_DOT, npb, nb, 4 * nb)
    a, b = mixed(rng, (nb, npb)), mixed(rng, (nb, npb))
    ad, bd = E.fd(a), E.fd(b)

    def loss(mode):
        out = torch.full((nb,), float("nan"), device="cuda")
        ws, nws = ws_of(lib, DET_DIFF_LOSS, n=npb, c=nb)
        E.call(lib, K, "shdr_diff_loss_det_f32", P(ad), P(bd), P(out), P(ws), nws, nb, npb, mode)
        return out
    before = counter(lib)
    for mode in (0, 1):
        (got,) = five_equal(lambda: loss(mode), "diff_loss_det mode %d" % mode)
        d = a.astype(np.float64) - b.astype(np.float64)
        terms = np.abs(d) if mode else d * d
        # a term carries the rounding of the difference (twice in the square) and of the square: 3; the block's division and the fold: 2
        E.assert_bar(E.back(got), F.diff_loss(a, b, mode), F.sum_bar(terms, axis=1, extra=5) / npb, "diff_loss_det mode %d" % mode)
        assert rel_err(E.back(got), F.diff_loss(a, b, mode)) <= FWD_BAR
    ai, bi = E.ints(rng, (nb, npb), -4, 4), E.ints(rng, (nb, npb), -4, 4)
    aid, bid = E.fd(ai), E.fd(bi)

    def dot(second):
        out = torch.full((nb,), float("nan"), device="cuda")
        ws, nws = ws_of(lib, DET_SAMPLE_DOT, n=npb, c=nb)
        E.call(lib, K, "shdr_sample_dot_det_f32", P(aid), P(bid) if second else None, P(out), P(ws), nws, nb, npb)
        return out
    E.assert_equal(E.back(dot(False)), F.sample_dot(ai))
    E.assert_equal(E.back(dot(True)), F.sample_dot(ai, bi))

    def mdot():
        out = torch.full((nb,), float("nan"), device="cuda")
        ws, nws = ws_of(lib, DET_SAMPLE_DOT, n=npb, c=nb)
        E.call(lib, K, "shdr_sample_dot_det_f32", P(ad), P(bd), P(out), P(ws), nws, nb, npb)
        return out
    (got,) = five_equal(mdot, "sample_dot_det")
    prod = a.astype(np.float64) * b.astype(np.float64)
    E.assert_bar(E.back(got), prod.sum(axis=1), F.sum_bar(prod, axis=1, extra=3), "sample_dot_det")
    assert counter(lib) == before
    K.diff_loss(ad, bd, 0)
    K.sample_dot(ad)
    assert counter(lib) == before + 2


@pytest.mark.parametrize("shape", [(2, 9, 16, 3), (1, 16, 12, 4), (1, 211, 277, 3)], ids=str)       # 4, 3 and 512 (capped) blocks
def test_tv_loss(K, lib, shape):
    rng = np.random.default_rng(sum(shape))
    total = int(np.prod(shape))
    blocks = rows_of(lib, DET_TV_LOSS, total, 0, 4)
    assert blocks == min(-(-total // 256), 512) >= 2

    def tv(yd):
        out = torch.full((1,), float("nan"), device="cuda")
        ws, nws = ws_of(lib, DET_TV_LOSS, n=total)
        E.call(lib, K, "shdr_tv_loss_det_f32", P(yd), P(out), P(ws), nws, *shape)
        return out
    y = E.ints(rng, shape, -8, 8)
    ref = F.tv_loss(y)
    before = counter(lib)
    E.assert_bar(E.back(tv(E.fd(y))), [ref], F.bar32(blocks, ref), "tv_loss_det, integers: the bar of the default kernel's test")
    ym = mixed(rng, shape)
    (got,) = five_equal(lambda: tv(E.fd(ym)), "tv_loss_det")
    terms = np.concatenate([t.reshape(-1) for t in F.tv_terms(ym)])
    E.assert_bar(E.back(got), [F.tv_loss(ym)], F.sum_bar(terms, extra=4) / total, "tv_loss_det")
    assert rel_err(E.back(got), [F.tv_loss(ym)]) <= FWD_BAR
    assert counter(lib) == before
    K.tv_loss(E.fd(ym))
    assert counter(lib) == before + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_lin_frontend_bwd_det_f32: the gather form
# ---------------------------------------------------------------------------------------------------------------------------------
FRONT = [(1, 2, 2), (1, 2, 3), (1, 3, 2), (1, 3, 3), (2, 5, 7), (1, 7, 9), (2, 64, 64)]


@pytest.mark.parametrize("nhw", FRONT, ids=str)
def test_lin_frontend_bwd_gather(K, lib, nhw):
    rng = np.random.default_rng(nhw[1] * 11 + nhw[2])
    n, h, w = nhw
    img = E.front_image(rng, nhw)
    imgd = E.fd(img)

    def gather(dFd):
        out = torch.full(nhw + (3,), float("nan"), device="cuda")         # written once per element: no memset, nothing read
        before = counter(lib)
        E.call(lib, K, "shdr_lin_frontend_bwd_det_f32", P(imgd), P(dFd), P(out), n, h, w, dFd.shape[3])
        assert counter(lib) == before
        return out
    dF = E.ints(rng, nhw + (96,), -8, 8)
    dFd = E.fd(dF)
    got = gather(dFd)
    E.assert_equal(E.back(got), F.lin_frontend_bwd(img, dF), "integer gradients: exact")
    before = counter(lib)
    scatter = K.lin_frontend_bwd(imgd, dFd)
    assert counter(lib) == before + 1
    assert torch.equal(bits(got), bits(scatter)), "gather and scatter differ on integer gradients"
    E.assert_equal(E.back(gather(E.fd(dF[..., :93].copy()))), F.lin_frontend_bwd(img, dF), "93 channels")
    dF = E.f32(rng, nhw + (96,))
    (got,) = five_equal(lambda: gather(E.fd(dF)), "lin_frontend_bwd_det")
    E.assert_bar(E.back(got), F.lin_frontend_bwd(img, dF), F.bar32(43, F.lin_frontend_bwd(img, dF, absolute=True)), "the scatter test's bar")
    with K.deterministic(True):
        assert torch.equal(bits(K.lin_frontend_bwd(imgd, E.fd(dF))), bits(got))


# ---------------------------------------------------------------------------------------------------------------------------------
# the Python wrappers under K.deterministic(True)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_route_every_weight_gradient_family(K, lib):
    """K.conv2d_wgrad picks the Winograd-domain and split-operand kernels for deep layers; in deterministic mode every family runs its own
    slab form: the counter stands still, five runs agree on operands of mixed magnitude, the result is on the gradient bar, accumulating
    into g0 is g0 + the result; padded (3-channel) layers too"""
    rng = np.random.default_rng(5)
    for name, n, h, w, c1, c2, cout, k, stride in (("winograd_family_64_64", 2, 32, 32, 64, 0, 64, 3, 1), ("split_family_128_128", 2, 32, 32, 128, 0, 128, 3, 1),
                                                   ("two_sources_32_32_64", 2, 32, 32, 32, 32, 64, 3, 1), ("padded_head_16_3", 2, 32, 32, 16, 0, 3, 3, 1),
                                                   ("padded_image_3_16_k7", 2, 32, 32, 3, 0, 16, 7, 1)):
        x, dz = E.fd(mixed(rng, (n, h, w, c1))), E.fd(mixed(rng, (n, h // stride, w // stride, cout)))
        x2 = E.fd(mixed(rng, (n, h, w, c2))) if c2 else None
        shape = (k, k, c1 + c2, cout)
        ref = C.wgrad(E.back(x), None if x2 is None else E.back(x2), E.back(dz), shape, stride, 1.0 / 255, None)
        g0 = E.fd(mixed(rng, shape))
        if name.startswith(("winograd_family", "split_family")):       # these two run their own slab forms: at least two slabs each
            d = K._conv_desc(tuple(x.shape), shape, stride, c2, 1.0 / 255, None)
            op, slab = (DET_WINOGRAD, 16 * c1 * cout * 4) if name.startswith("winograd") else (DET_X3, k * k * c1 * cout * 4)
            assert lib.shdr_det_workspace_bytes(op, ctypes.byref(d), 0, 0, 0) >= 2 * slab, name
        before = counter(lib)
        K.conv2d_wgrad(x, x2, dz, shape, stride, 1.0 / 255)
        moved = counter(lib) - before
        with K.deterministic(True):
            before = counter(lib)
            (dw,) = five_equal(lambda: K.conv2d_wgrad(x, x2, dz, shape, stride, 1.0 / 255), name)
            acc = K.conv2d_wgrad(x, x2, dz, shape, stride, 1.0 / 255, out=g0.clone())
            assert counter(lib) == before, name
        err = rel_err(E.back(dw), ref)
        print("%s: default path moved the counter by %d; deterministic %.3e of float64" % (name, moved, err))
        assert err <= GRAD_BAR, name
        assert torch.equal(acc, g0 + dw), name


def test_refusals(K, lib):
    d = W.desc_of(K, (1, 47, 45, 32), 0, 3, 32, 1)
    x, dz = torch.zeros((1, 47, 45, 32), device="cuda"), torch.zeros((1, 47, 45, 32), device="cuda")
    buf, v = W.guarded(9 * 32 * 32)
    dw = v.view(torch.float32)
    ws, nws = ws_of(lib, DET_WGRAD, d, c=0)
    st = K._stream()
    assert lib.shdr_conv2d_wgrad_det_f32(ctypes.byref(d), P(x), 0, P(dz), P(dw), None, nws, st) == W.E_NULL
    assert lib.shdr_conv2d_wgrad_det_f32(ctypes.byref(d), P(x), 0, P(dz), P(dw), P(ws), nws - 4, st) == W.E_SHAPE
    assert b"needed" in lib.shdr_last_error()
    assert lib.shdr_conv2d_wgrad_det_f32(ctypes.byref(d), P(x), 0, P(dz), P(dw), P(ws, 4), nws, st) == W.E_ALIGN
    assert lib.shdr_conv2d_wgrad_det_f32(ctypes.byref(d), P(x), 1, P(dz), P(dw), P(ws), nws, st) == W.E_SHAPE            # no second source
    for algo in (W.MFMA_F16, W.MFMA_BF16, W.AUTO_F16):
        d.algo = algo
        assert lib.shdr_conv2d_wgrad_det_f32(ctypes.byref(d), P(x), 0, P(dz), P(dw), P(ws), nws, st) == W.E_SHAPE
        assert lib.shdr_det_workspace_bytes(DET_WGRAD, ctypes.byref(d), 0, 0, 0) == -1
    W.untouched(buf, "refused deterministic weight gradients")
    assert lib.shdr_apply_rf_bwd_det_f32(P(x), P(x), P(x), P(dw), None, P(ws), nws, 1, 16, 8192, st) == W.E_SHAPE           # K <= 4096
    assert lib.shdr_bias_grad_det_f32(P(dz), P(dw), P(ws), 4, 2115, 32, st) == W.E_SHAPE
    assert lib.shdr_act_bwd_bias_det_f32(P(dz), None, None, P(dw), None, 2115, 32, 0, st) == W.E_NULL
    W.untouched(buf, "refused deterministic calls")
