"""The up-sampling 3x3 layers with the channel mix at low resolution (csrc/up2_lowres.hip; K.conv2d_up2(..., lowres=True)): a 1x1 GEMM
Cin -> 9 Cout on the low-res input (conv_x3_1x1_kernel) and the stencil pass that sums the nine tap planes with the bilinear weights.
Checked against the float64 oracle (resize, then conv) at the bar of tests/test_gpu_ops.py, against today's path at the bar
tests/test_gpu_switches.py sets between two fp32-grade kernels, and for its range slot, determinism, switch, launches and fall-back.
SHDR_X3_MIN_BLOCKS=1 takes the fill-the-chip threshold (speed only) of the low-res GEMM out of the way.
The per-element comparison with a float64 model of the two launches is tests/test_gpu_up2_lowres_exact.py."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import ops

pytestmark = pytest.mark.gpu

TOL = 1e-5            # tests/test_gpu_ops.py
TOL_PATHS = 5e-6      # tests/test_gpu_switches.py: two fp32-grade kernels on the same input

# low-res (N, h, w, Cin, Cout)
SHAPES = [
    (2, 1, 1, 64, 128),       # one-pixel source: every tap clamped and most taps outside
    (1, 1, 7, 64, 64),        # one-row image
    (1, 6, 1, 64, 64),        # one-column image
    (2, 9, 10, 96, 128),      # three chunks, 1152 columns
    (1, 17, 15, 160, 256),    # ragged against the 128-pixel GEMM blocks and the stencil pass's 16-column strips
    (1, 5, 33, 64, 64),       # 576 columns: the padding route
    (1, 8, 8, 512, 512),      # sixteen chunks, 4608 columns
]
EPILOGUES = ["none", "bias_relu", "up_block"]
_CACHE = {}


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _act(v, act):
    return {0: lambda t: t, 1: ops.relu, 2: ops.leaky_relu}[act](v)


def _case(shape, mag=1.0):
    """inputs of a shape and the float64 pre-epilogue convolution of the up-sampled image, computed once"""
    key = (shape, mag)
    if key not in _CACHE:
        n, h, w, cin, cout = shape
        rng = np.random.default_rng(sum(shape) + 5)
        x = _f32(rng.normal(size=(n, h, w, cin)) * mag)
        wt = _f32(rng.normal(size=(3, 3, cin, cout)) / np.sqrt(9 * cin))
        b, sc, sh = _f32(rng.normal(size=cout) * mag), _f32(rng.uniform(0.5, 1.5, cout)), _f32(rng.normal(size=cout) * mag)
        conv = ops.conv2d(ops.resize_bilinear_2x(x.astype(np.float64)), wt.astype(np.float64))
        conv.setflags(write=False)
        _CACHE[key] = (x, wt, b, sc, sh, conv)
    return _CACHE[key]


def _epilogue_args(K, case, epi, act2=None):
    x, wt, b, sc, sh, conv = case
    if epi == "none":
        return {}, conv
    if epi == "bias_relu":
        return dict(bias=_dev(b), act1=K.ACT_RELU), ops.relu(conv + b.astype(np.float64))
    a2 = K.ACT_RELU if act2 is None else act2
    ref = _act(ops.relu(conv + b.astype(np.float64)) * sc.astype(np.float64) + sh.astype(np.float64), a2)
    return dict(bias=_dev(b), act1=K.ACT_RELU, scale=_dev(sc), shift=_dev(sh), act2=a2), ref


def _run(K, case, kw, lowres=True):
    with torch.no_grad():
        x = _dev(case[0])
        K.absmax_slot(x)
        y = K.conv2d_up2(x, _dev(case[1]), **kw) if lowres is None else K.conv2d_up2(x, _dev(case[1]), lowres=lowres, **kw)
    torch.cuda.synchronize()
    return y


def _force(monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.delenv("SHDR_NO_UP2_LOWRES", raising=False)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _kernels(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events()}


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_up2_lowres_vs_float64_oracle_and_todays_path(shdr, monkeypatch, shape, epi):
    K = shdr._ops
    _force(monkeypatch)
    case = _case(shape)
    kw, ref = _epilogue_args(K, case, epi)
    y = _run(K, case, kw)
    err = rel_err(y.cpu().numpy(), ref)
    old = _run(K, case, kw, lowres=None)
    diff = rel_err(y.cpu().numpy(), old.cpu().numpy())
    print("up2_lowres %s %s: vs oracle %.3g, vs today's path %.3g" % (shape, epi, err, diff))
    assert tuple(y.shape) == ref.shape and err <= TOL, err
    assert diff <= TOL_PATHS, diff
    # the range slot holds exactly the output's maximum
    assert float(K._range_of(y)) == float(y.abs().max())


def test_up2_lowres_lrelu_as_second_activation(shdr, monkeypatch):
    K = shdr._ops
    _force(monkeypatch)
    case = _case((2, 9, 10, 96, 128))
    kw, ref = _epilogue_args(K, case, "up_block", act2=K.ACT_LRELU)
    y = _run(K, case, kw)
    assert (ref < 0).any()
    assert rel_err(y.cpu().numpy(), ref) <= TOL
    assert rel_err(y.cpu().numpy(), _run(K, case, kw, lowres=None).cpu().numpy()) <= TOL_PATHS
    assert float(K._range_of(y)) == float(y.abs().max())


@pytest.mark.parametrize("mag", [1e-3, 1e3])
def test_up2_lowres_range_guard(shdr, monkeypatch, mag):
    """inputs far from unit scale: the GEMM scales its input by the range slot, so the bar against the oracle is the same"""
    K = shdr._ops
    _force(monkeypatch)
    case = _case((1, 17, 15, 160, 256), mag)
    for epi in ("none", "up_block"):
        kw, ref = _epilogue_args(K, case, epi)
        y = _run(K, case, kw)
        assert rel_err(y.cpu().numpy(), ref) <= TOL
        assert float(K._range_of(y)) == float(y.abs().max())


def test_up2_lowres_is_deterministic(shdr, monkeypatch):
    K = shdr._ops
    _force(monkeypatch)
    for shape in ((1, 17, 15, 160, 256), (2, 9, 10, 96, 128)):
        case = _case(shape)
        kw, _ = _epilogue_args(K, case, "up_block")
        assert _bits_equal(_run(K, case, kw), _run(K, case, kw))


def test_up2_lowres_rows_per_segment_do_not_change_the_bits(shdr, monkeypatch):
    """the stencil pass walks row segments whose length follows the grid size: a pixel's sums are the same in any segment"""
    K = shdr._ops
    _force(monkeypatch)
    case = _case((1, 17, 15, 160, 256))
    kw, _ = _epilogue_args(K, case, "up_block")
    y = _run(K, case, kw)
    for rows in ("1", "5", "32"):
        monkeypatch.setenv("SHDR_UP2_LOWRES_ROWS", rows)
        assert _bits_equal(_run(K, case, kw), y), rows


def test_up2_lowres_gemm_column_padding_does_not_change_the_bits(shdr, monkeypatch):
    """1152 tap columns run as nine 128-cout blocks or, padded to 1280, as five 256-cout blocks of conv_x3_1x1_kernel: bit-identical
    forms of the GEMM (tests/test_gpu_x3_1x1.py), and the stencil pass never reads the padding"""
    K = shdr._ops
    _force(monkeypatch)
    case = _case((2, 9, 10, 96, 128))
    kw, ref = _epilogue_args(K, case, "up_block")
    monkeypatch.setenv("SHDR_UP2_LOWRES_PAD", "128")
    names = _kernels(lambda: _run(K, case, kw))
    assert any("conv_x3_1x1_kernel<2>" in k for k in names), names
    y128 = _run(K, case, kw)
    monkeypatch.setenv("SHDR_UP2_LOWRES_PAD", "256")
    names = _kernels(lambda: _run(K, case, kw))
    assert any("conv_x3_1x1_kernel<4>" in k for k in names), names
    y256 = _run(K, case, kw)
    assert _bits_equal(y128, y256)
    assert rel_err(y256.cpu().numpy(), ref) <= TOL


def test_up2_lowres_switch_gives_todays_bits(shdr, monkeypatch):
    K = shdr._ops
    _force(monkeypatch)
    case = _case((2, 9, 10, 96, 128))
    kw, _ = _epilogue_args(K, case, "up_block")
    old = _run(K, case, kw, lowres=None)
    new = _run(K, case, kw)
    monkeypatch.setenv("SHDR_NO_UP2_LOWRES", "1")
    off = _run(K, case, kw)
    assert _bits_equal(off, old)
    assert not _bits_equal(new, old)         # (the keyword did select another form)


def test_up2_lowres_kernels_launched(shdr, monkeypatch):
    K = shdr._ops
    _force(monkeypatch)
    case = _case((2, 9, 10, 96, 128))
    kw, _ = _epilogue_args(K, case, "up_block")
    _run(K, case, kw), _run(K, case, kw, lowres=None)                    # filters prepared
    new = _kernels(lambda: _run(K, case, kw))
    assert any("conv_x3_1x1_kernel" in k for k in new), new
    assert any("up2_lowres_stencil_kernel" in k for k in new), new
    assert not any("resize2x_kernel" in k for k in new), new
    assert not any("conv_x3_" in k and "<true" in k for k in new), new
    old = _kernels(lambda: _run(K, case, kw, lowres=None))
    assert any("conv_x3_" in k and "<true" in k for k in old), old
    assert not any("up2_lowres" in k or "conv_x3_1x1_kernel" in k for k in old), old
    assert old == _kernels(lambda: _run(K, case, kw, lowres=False))


@pytest.mark.parametrize("shape", [(1, 8, 8, 32, 64), (1, 8, 8, 64, 32), (1, 9, 8, 64, 64)], ids=["cin32", "cout32", "odd"])
def test_up2_lowres_refused_shapes_fall_back_bit_for_bit(shdr, monkeypatch, shape):
    """Cin 32, Cout 32 and an odd up-sampled size are not taken: the call is today's.  (2x up-sampling of a tensor always gives even sizes, so
    the odd case asks the predicate itself.)"""
    K = shdr._ops
    _force(monkeypatch)
    n, h, w, cin, cout = shape
    lib = shdr._lib.load()
    d = shdr._lib.ConvDesc()
    d.N, d.H, d.W, d.C1, d.Cout, d.KH, d.KW, d.stride = n, 2 * h, 2 * w, cin, cout, 3, 3, 1
    d.pad_t, d.pad_l, d.Ho, d.Wo, d.x2_scale, d.prologue, d.cout_valid = 1, 1, 2 * h, 2 * w, 1.0, K.PROLOGUE_BILINEAR2X, cout
    if h % 2:
        d.H = d.Ho = 2 * h - 1
        assert lib.shdr_conv2d_up2_lowres_ok_f32(ctypes.byref(d)) == 0
        d.H = d.Ho = 2 * h
        assert lib.shdr_conv2d_up2_lowres_ok_f32(ctypes.byref(d)) == 1
        return
    assert lib.shdr_conv2d_up2_lowres_ok_f32(ctypes.byref(d)) == 0
    case = _case(shape)
    kw, _ = _epilogue_args(K, case, "up_block")
    assert _bits_equal(_run(K, case, kw), _run(K, case, kw, lowres=None))


def test_up2_lowres_fallbacks_in_python(shdr, monkeypatch):
    """with EXACT_FP32 and under a gradient tape the keyword changes nothing"""
    K = shdr._ops
    _force(monkeypatch)
    case = _case((2, 9, 10, 96, 128))
    kw, _ = _epilogue_args(K, case, "bias_relu")
    monkeypatch.setattr(K, "EXACT_FP32", True)
    assert _bits_equal(_run(K, case, kw), _run(K, case, kw, lowres=None))
    monkeypatch.setattr(K, "EXACT_FP32", False)
    x, wt = _dev(case[0]), _dev(case[1]).requires_grad_(True)
    names = _kernels(lambda: K.conv2d_up2(x, wt, lowres=True))
    assert not any("up2_lowres" in k for k in names), names


def test_hallucination_net_decoder_takes_the_lowres_form(shdr, monkeypatch):
    """tape-free fp32 inference of an `up` block selects the form; SHDR_NO_UP2_LOWRES=1 gives the block's former bits"""
    K = shdr._ops
    _force(monkeypatch)
    torch.manual_seed(3)
    blk = shdr.hallucination_net.up(64, 64)
    x = torch.randn(1, 8, 8, 64, device="cuda")
    with torch.no_grad():
        K.absmax_slot(x)
        names = _kernels(lambda: blk.call(x, training=False))
        assert any("up2_lowres_stencil_kernel" in k for k in names), names
        y = blk.call(x, training=False)
        scale, shift = blk.norm1.folded()
        old = K.conv2d_up2(x, blk.conv1.kernel, blk.conv1.bias, act1=K.ACT_RELU, scale=scale, shift=shift, act2=K.ACT_RELU)
        assert rel_err(y.cpu().numpy(), old.cpu().numpy()) <= TOL_PATHS
        monkeypatch.setenv("SHDR_NO_UP2_LOWRES", "1")
        assert _bits_equal(blk.call(x, training=False), old)
