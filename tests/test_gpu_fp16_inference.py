"""Native-fp16 INFERENCE (`Inference(..., precision="fp16")`, shdr_conv2d_fwd_fused_f16) against the float64 ORACLE.

The fp16 forward kernels take the inference epilogue y = act2(affine(act1(conv + bias)) + residual) as a compile-time option: the folded
BatchNorm and second activation of the Hallucination-Net (`conv1`, the `up` blocks, the composed s1 -> conv2 -> norm2 tail) and the residual
heads of the Dequantization- / Refinement-Net.  Bars (unit round-off u = 2^-11; operands and stored feature maps are fp16, accumulation and
epilogue fp32):
  * one layer, each kernel family forced with the library's switches: max|err| <= 3e-3 * max|reference| (the fp16 layer bar of
    test_gpu_fp16_oracle.py);
  * whole networks and the inference chain: 2e-2 of the tensor scale (the fine-tuning chain's intermediate bar);
  * properties: deterministic, graph replay bit-identical to eager, batch independence, precision scoped to the call, finite and >= 0.
Measured on MI355X: whole nets deq 2.8e-4, hal 3.4e-4, ref 3.4e-4; golden chain C_pred 2.0e-4, invcrf 2.4e-6, B_pred 6.5e-4,
hal 4.1e-4, A_pred 1.7e-3, hdr 1.6e-3 -- well inside the 2e-2 bar, which stays the fine-tuning chain's.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import torch_ref as R
from conftest import GOLDEN, quantised_image, rel_err
from oracle import nets, ops

pytestmark = pytest.mark.gpu
LAYER_TOL = 3e-3
NET_TOL = 2e-2


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().to(dtype)


def host(t):
    return t.detach().float().cpu().numpy()


def as_f16(x):
    """the values an fp16 tensor holds (the reference is computed from them)"""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float64)


ACTS = {0: lambda z: z, 1: torch.relu, 2: R.lrelu, 3: torch.tanh}

# name, N, H, W, C1, C2, Cout (gemm), cout_valid (None: fp16 output), k, act1, affine, residual ("f32" / "f16" / None, cstride), act2,
# kernel families the case runs on
CASES = [
    ("up_3x3_64_64_bn_relu", 2, 21, 37, 64, 0, 64, None, 3, 1, True, (None, 0), 1, ("w3", "general")),
    ("conv1_3x3_512_512_bn_relu", 1, 9, 11, 512, 0, 512, None, 3, 0, True, (None, 0), 1, ("w3", "general")),
    ("skip_1x1_64_64_bn_relu", 2, 17, 13, 64, 64, 64, None, 1, 0, True, (None, 0), 1, ("general",)),
    ("fp16_out_residual_lrelu", 1, 19, 23, 32, 32, 64, None, 3, 1, True, ("f16", 64), 2, ("general",)),
    ("deq_head_tanh_f32_residual", 2, 13, 19, 16, 0, 16, 3, 3, 3, False, ("f32", 3), 0, ("patch", "general")),
    ("ref_head_relu_f16_residual", 2, 21, 35, 16, 0, 16, 3, 3, 0, False, ("f16", 16), 1, ("patch", "general")),
    ("hal_tail_1x1_64_64_3_bn_relu", 2, 18, 30, 64, 64, 16, 3, 1, 0, True, (None, 0), 1, ("general",)),
]
CASE_IDS = [(c, fam) for c in CASES for fam in c[-1]]


def _force(monkeypatch, family):
    if family == "w3":
        monkeypatch.setenv("SHDR_W3_MIN_BLOCKS", "0")
    elif family == "general":
        monkeypatch.setenv("SHDR_NO_PATCH", "1")
        monkeypatch.setenv("SHDR_NO_W3", "1")


@pytest.mark.parametrize("case,family", CASE_IDS, ids=["%s-%s" % (c[0], f) for c, f in CASE_IDS])
def test_fused_fp16_layer_vs_float64(shdr, case, family, monkeypatch):
    name, n, h, w, c1, c2, cout, cv, k, act1, affine, (res_kind, res_cs), act2, _ = case
    _force(monkeypatch, family)
    K = shdr._ops
    rng = np.random.default_rng(len(name) * 7 + h)
    x = as_f16(rng.normal(size=(n, h, w, c1)))
    x2 = as_f16(rng.normal(size=(n, h, w, c2))) if c2 else None
    nout = cv or cout
    wt = np.zeros((k, k, c1 + c2, cout), np.float32)
    wt[..., :nout] = rng.normal(size=(k, k, c1 + c2, nout)) / np.sqrt(k * k * (c1 + c2))
    b = (rng.normal(size=nout) * 0.1).astype(np.float32)
    sc = (rng.random(nout) * 1.5 + 0.25).astype(np.float32) if affine else None
    sh = (rng.normal(size=nout) * 0.3).astype(np.float32) if affine else None
    res = None
    if res_kind:
        res = rng.normal(size=(n, h, w, res_cs))
        res = as_f16(res) if res_kind == "f16" else res.astype(np.float32).astype(np.float64)
    # float64 reference
    xin = x if x2 is None else np.concatenate([x, x2], -1)
    z = R.conv2d(R.T(xin), R.T(wt[..., :nout]), R.T(b))
    y = ACTS[act1](z)
    if affine:
        y = y * R.T(sc) + R.T(sh)
    if res is not None:
        y = y + R.T(res[..., :nout])
    y = ACTS[act2](y).numpy()
    # the layer's kernel family: the library's own predicates, as its dispatcher asks them
    d = K._conv_desc_h((n, h, w, c1), c2, (k, k), cout, 1, cv)
    lib = shdr._lib.load()
    if family == "w3":
        assert lib.shdr_conv2d_w3_ok_f16(ctypes.byref(d)) == 1
    elif family == "patch":
        assert lib.shdr_conv2d_patch_ok_f16(ctypes.byref(d)) == 1
    calls = K.FUSED_F16_CALLS[0]
    with torch.no_grad():
        yy = K.conv2d(dev(x, K.HALF), dev(wt), dev(b), x2=None if x2 is None else dev(x2, K.HALF), act1=act1,
                      scale=None if sc is None else dev(sc), shift=None if sh is None else dev(sh),
                      residual=None if res is None else dev(res, K.HALF if res_kind == "f16" else torch.float32), act2=act2,
                      cout_valid=cv)
    assert K.FUSED_F16_CALLS[0] == calls + 1
    assert yy.dtype == (torch.float32 if cv else torch.float16) and tuple(yy.shape) == y.shape
    assert rel_err(host(yy), y) <= LAYER_TOL


def test_fused_fp16_refusals(shdr):
    """what the mode does not take is refused loudly, never dropped"""
    K = shdr._ops
    x = torch.zeros((1, 8, 8, 64), device="cuda", dtype=K.HALF)
    w = torch.zeros((3, 3, 64, 64), device="cuda")
    s = torch.ones(64, device="cuda")
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            K.conv2d(x, w, pad=(1, 1), scale=s)
        with pytest.raises(RuntimeError, match="tanh"):               # tanh is compiled into the fp32-output heads only
            K.conv2d(x, w, act1=K.ACT_TANH, scale=s)
    wg = w.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):                           # on a gradient tape: bias + act1 only, as before
        K.conv2d(x, wg, scale=s)


def test_fused_fp16_entry_through_ctypes_only(shdr):
    """shdr_conv2d_fwd_fused_f16 bound with ctypes alone (no _ops): 3x3 32 -> 16 (3 stored) fp32 head, folded affine, fp32 residual
    with channel stride 5, relu -- against NumPy"""
    from test_gpu_abi import ConvDesc
    L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "singlehdr-tf2_amd", "libshdr.so"))
    P, V, I = ctypes.POINTER(ConvDesc), ctypes.c_void_p, ctypes.c_int
    L.shdr_conv2d_fwd_fused_f16.restype, L.shdr_conv2d_fwd_fused_f16.argtypes = I, [P] + [V] * 7 + [I, V, I, V]
    L.shdr_conv2d_packed_filter_elems_f16.restype, L.shdr_conv2d_packed_filter_elems_f16.argtypes = ctypes.c_int64, [I] * 5
    L.shdr_conv2d_pack_filter_f16.restype, L.shdr_conv2d_pack_filter_f16.argtypes = I, [V, V] + [I] * 5 + [ctypes.c_float, V]
    rng = np.random.default_rng(3)
    n, h, w, cin, cout, cv = 1, 10, 14, 32, 16, 3
    x = rng.normal(size=(n, h, w, cin)).astype(np.float16)
    wt = np.zeros((3, 3, cin, cout), np.float32)
    wt[..., :cv] = rng.normal(size=(3, 3, cin, cv)) / np.sqrt(9 * cin)
    b, sc, sh = (rng.normal(size=cv).astype(np.float32) for _ in range(3))
    res = rng.normal(size=(n, h, w, 5)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    wd, bd, scd, shd, rd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (wt, b, sc, sh, res))
    wp = torch.empty(int(L.shdr_conv2d_packed_filter_elems_f16(3, 3, cin, 0, cout)), device="cuda", dtype=torch.float16)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.shdr_conv2d_pack_filter_f16(V(wd.data_ptr()), V(wp.data_ptr()), 3, 3, cin, 0, cout, 1.0, stream) == 0
    y = torch.empty((n, h, w, cv), device="cuda")
    d = ConvDesc(N=n, H=h, W=w, C1=cin, C2=0, Cout=cout, KH=3, KW=3, stride=1, pad_t=1, pad_l=1, Ho=h, Wo=w, x2_scale=1.0,
                 act1=0, act2=1, res_cstride=5, cout_valid=cv)
    rc = L.shdr_conv2d_fwd_fused_f16(ctypes.byref(d), V(xd.data_ptr()), None, V(wp.data_ptr()), V(bd.data_ptr()), V(scd.data_ptr()),
                                     V(shd.data_ptr()), V(rd.data_ptr()), 1, V(y.data_ptr()), 1, stream)
    assert rc == 0
    torch.cuda.synchronize()
    z = ops.conv2d(x.astype(np.float64), wt[..., :cv].astype(np.float64), b.astype(np.float64), 1)
    want = np.maximum(z * sc + sh + res[..., :cv], 0.0)
    assert rel_err(y.cpu().numpy(), want) <= LAYER_TOL


def _models(shdr, seeds):
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    P = {k: nets.init_params(getattr(nets, k + "_spec")(), s) for k, s in seeds.items()}
    return {k: getattr(shdr, mods[k]).model().load_numpy(P[k]) for k in P}, P


def test_fp16_inference_networks_vs_float64(shdr):
    """deq, hal, ref with training=False under precision("fp16") (randomised BatchNorm statistics: nets.init_params) against the
    oracle; the fused fp16 entry really ran (one head each for deq / ref; conv1, the five `up` blocks and the tail for hal) and the
    feature maps are fp16"""
    K = shdr._ops
    ms, P = _models(shdr, dict(deq=71, hal=72, ref=73))
    rng = np.random.default_rng(70)
    x = quantised_image(rng, (2, 64, 96, 3))
    abc = [rng.random((2, 64, 64, 3)) for _ in range(3)]
    dtypes = []
    orig_h = K.conv2d_h

    def spy(x, *a, **kw):
        dtypes.append(x.dtype)
        return orig_h(x, *a, **kw)

    K.conv2d_h = spy
    try:
        with torch.no_grad(), K.precision("fp16"):
            c0 = K.FUSED_F16_CALLS[0]
            y_deq = ms["deq"](dev(x), training=False)
            c1 = K.FUSED_F16_CALLS[0]
            y_hal = ms["hal"](dev(x), training=False)
            c2 = K.FUSED_F16_CALLS[0]
            y_ref = ms["ref"](K.pack3([dev(t) for t in abc], 16, K.HALF), training=False)
            c3 = K.FUSED_F16_CALLS[0]
    finally:
        K.conv2d_h = orig_h
    assert (c1 - c0, c2 - c1, c3 - c2) == (1, 7, 1)
    assert dtypes and all(t == torch.float16 for t in dtypes)
    assert K.PRECISION == "fp32"
    errs = dict(deq=rel_err(host(y_deq), nets.deq_forward(P["deq"], x)),
                hal=rel_err(host(y_hal), nets.hal_forward(P["hal"], x)),
                ref=rel_err(host(y_ref), nets.ref_forward(P["ref"], np.concatenate(abc, -1))))
    print("fp16 inference, whole nets vs float64:", errs)
    assert max(errs.values()) <= NET_TOL, errs
    assert (host(y_hal) >= 0).all() and (host(y_ref) >= 0).all()


def test_fp16_inference_chain_matches_golden(shdr):
    """Inference(..., precision="fp16") on the committed fixture: every intermediate within the bar, deterministic, precision restored"""
    K = shdr._ops
    g = np.load(os.path.join(GOLDEN, "inference_64.npz"))
    ms, _ = _models(shdr, {k: int(g["seed_" + k]) for k in ("deq", "lin", "hal", "ref")})
    run = shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision="fp16")
    calls = K.FUSED_F16_CALLS[0]
    out = run(dev(g["ldr"]), return_intermediates=True)
    assert K.FUSED_F16_CALLS[0] - calls == 9                 # deq head, hal conv1 + 5 up + tail, ref head
    assert K.PRECISION == "fp32"
    errs = {k: rel_err(host(out[k]), g[k]) for k in ("C_pred", "invcrf", "B_pred", "hal", "A_pred", "hdr")}
    print("fp16 inference chain vs golden (float64 oracle):", errs)
    assert max(errs.values()) <= NET_TOL, errs
    hdr = run(dev(g["ldr"]))
    np.testing.assert_array_equal(host(hdr), host(out["hdr"]))          # deterministic
    assert bool(torch.isfinite(hdr).all()) and float(hdr.min()) >= 0.0
    assert K.PRECISION == "fp32"
    with pytest.raises(ValueError):
        shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision="bf16")


def test_fp16_graphed_inference_equals_eager(shdr):
    ms, _ = _models(shdr, dict(deq=80, lin=81, hal=82, ref=83))
    eager = shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision="fp16")
    graphed = shdr.pipeline.GraphedInference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision="fp16")
    rng = np.random.default_rng(9)
    for _ in range(2):
        x = dev(quantised_image(rng, (1, 128, 96, 3)))
        np.testing.assert_array_equal(host(graphed(x)), host(eager(x)))
    assert shdr._ops.PRECISION == "fp32"


def test_fp16_inference_batch_independence_256(shdr, monkeypatch):
    """images in a batch do not interact.  The fp16 kernel families are chosen by shape (the wide 3x3 one also by how many blocks fill
    the chip: its threshold is lifted here so that both batches take the same kernels) and the fp32 Linearization-Net runs its exact
    kernels: one image alone and in a batch of three are bit-identical"""
    monkeypatch.setenv("SHDR_W3_MIN_BLOCKS", "0")
    monkeypatch.setattr(shdr._ops, "EXACT_FP32", True)
    ms, _ = _models(shdr, dict(deq=30, lin=31, hal=32, ref=33))
    streams = shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision="fp16", streams=3)
    run = shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision="fp16")
    x = dev(quantised_image(np.random.default_rng(6), (3, 256, 256, 3)))
    full = run(x)
    assert torch.equal(run(x[1:2].contiguous()), full[1:2])
    assert torch.equal(streams(x), full)                                # the multi-stream path: one image per stream
    assert shdr._ops.PRECISION == "fp32"
    assert bool(torch.isfinite(full).all()) and float(full.min()) >= 0.0
