"""The wide-block 1x1 split-operand kernel (conv_x3_1x1_kernel, csrc/conv_x3.hip) against the 64-cout instantiation it replaces
(SHDR_X3_1X1_SLICED=1): the same operands, chunk order, MFMA order and epilogue, so y and the output range slot are bit-identical"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, C1, C2, Cout, stride, residual): the 1x1 layers of the Linearization-Net's ResNet blocks and the Hallucination-Net's skip
# layers at N = 1, then Cout 32 / 64 / 128 / 256 / 512, two sources, stride 2 on odd sizes, pixel counts off the 128-pixel block
NETWORK = [
    (1, 128, 128, 64, 0, 256, 1, False), (1, 128, 128, 64, 0, 64, 1, False), (1, 128, 128, 64, 0, 256, 1, True),
    (1, 128, 128, 256, 0, 64, 1, False), (1, 128, 128, 64, 0, 256, 1, True),
    (1, 128, 128, 256, 0, 512, 2, False), (1, 128, 128, 256, 0, 128, 2, False),
    (1, 64, 64, 128, 0, 512, 1, True), (1, 64, 64, 512, 0, 128, 1, False), (1, 64, 64, 128, 0, 512, 1, True),
    (1, 32, 32, 512, 512, 512, 1, False), (1, 64, 64, 512, 512, 512, 1, False),
    (1, 128, 128, 256, 256, 256, 1, False), (1, 256, 256, 128, 128, 128, 1, False),
]
ENVELOPE = [
    (2, 20, 24, 64, 0, 32, 1, False), (1, 17, 19, 64, 0, 64, 1, True), (1, 17, 19, 96, 0, 128, 1, True),
    (3, 13, 11, 64, 32, 256, 1, True), (2, 9, 7, 128, 0, 512, 1, False), (1, 31, 33, 64, 0, 256, 2, False),
    (2, 45, 27, 192, 0, 128, 2, False), (1, 5, 5, 64, 64, 256, 1, False), (1, 1, 3, 32, 32, 128, 1, True),
]


def _layer(shape, seed, xscale=1.0, special=False):
    n, h, w, c1, c2, cout, stride, has_res = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c1, generator=g) * xscale
    x2 = torch.randn(n, h, w, c2, generator=g) * 255.0 * xscale if c2 else None
    if special:
        x.view(-1)[::997] = float("inf")
        x.view(-1)[5::1013] = -float("inf")
    wt = torch.randn(1, 1, c1 + c2, cout, generator=g) / np.sqrt(c1 + c2)
    b, sc, sh = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    ho, wo = (h + 1) // 2 if stride == 2 else h, (w + 1) // 2 if stride == 2 else w
    res = torch.randn(n, ho, wo, cout, generator=g) if has_res else None
    return [None if t is None else t.cuda() for t in (x, x2, wt, b, sc, sh, res)]


def _run(K, shape, tensors, act1=None):
    n, h, w, c1, c2, cout, stride, has_res = shape
    x, x2, wt, b, sc, sh, res = tensors
    x2s = 1.0 / 255 if c2 else 1.0
    assert K.conv2d_plan((n, h, w, c1), tuple(wt.shape), c2=c2, stride=stride, x2_scale=x2s, has_residual=has_res) == "x3"
    with torch.no_grad():
        xi, x2i = x.clone(), None if x2 is None else x2.clone()      # fresh tensors: fresh range slots
        K.absmax_slot(xi)
        if x2i is not None:
            K.absmax_slot(x2i)
        y = K.conv2d(xi, wt, b, stride=stride, x2=x2i, x2_scale=x2s, act1=K.ACT_RELU if act1 is None else act1, scale=sc, shift=sh, residual=res,
                     act2=K.ACT_LRELU if has_res else K.ACT_NONE)
    torch.cuda.synchronize()
    slot = K._range_of(y)
    assert slot is not None
    return y.cpu(), slot.cpu().view(torch.int32).clone()


def _both(shdr, monkeypatch, shape, act1=None, **kw):
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    tensors = _layer(shape, seed=sum(shape[:6]) + 3, **kw)
    monkeypatch.delenv("SHDR_X3_1X1_SLICED", raising=False)
    y1, r1 = _run(K, shape, tensors, act1)
    monkeypatch.setenv("SHDR_X3_1X1_SLICED", "1")
    y0, r0 = _run(K, shape, tensors, act1)
    monkeypatch.delenv("SHDR_X3_1X1_SLICED")
    return y1, r1, y0, r0


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("shape", NETWORK + ENVELOPE)
def test_x3_1x1_wide_block_is_bit_identical(shdr, monkeypatch, shape):
    y1, r1, y0, r0 = _both(shdr, monkeypatch, shape)
    assert _bits_equal(y1, y0), "max |diff| %g" % (y1 - y0).abs().max().item()
    assert torch.equal(r1, r0)


@pytest.mark.parametrize("xscale", [1e5, 1e-7])
@pytest.mark.parametrize("shape", [(1, 33, 35, 128, 128, 256, 1, True), (1, 29, 31, 256, 0, 512, 2, False)])
def test_x3_1x1_wide_block_is_bit_identical_at_range_ends(shdr, monkeypatch, shape, xscale):
    y1, r1, y0, r0 = _both(shdr, monkeypatch, shape, xscale=xscale)
    assert _bits_equal(y1, y0)
    assert torch.equal(r1, r0)


def test_x3_1x1_wide_block_non_finite_inputs(shdr, monkeypatch):
    # no ReLU in front of the affine map: it would turn the NaNs (inf - inf inside a dot product) into zeros
    y1, r1, y0, r0 = _both(shdr, monkeypatch, (1, 21, 23, 64, 64, 256, 1, True), act1=shdr._ops.ACT_NONE, special=True)
    assert not torch.isfinite(y1).all()
    assert _bits_equal(y1, y0)              # (NaNs included: the same bit patterns)
    assert torch.equal(r1, r0)


def test_x3_1x1_wide_block_vs_float64(shdr, monkeypatch):
    """the exact-fp32 bar of the split-operand kernels (1e-5) against a float64 reference"""
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    shape = (2, 37, 29, 128, 128, 256, 1, True)
    x, x2, wt, b, sc, sh, res = _layer(shape, seed=11)
    y, _ = _run(K, shape, (x, x2, wt, b, sc, sh, res))
    xd = torch.cat([x.double(), x2.double() / 255.0], dim=3).cpu()
    z = torch.relu(xd @ wt.double().cpu()[0, 0] + b.double().cpu()) * sc.double().cpu() + sh.double().cpu() + res.double().cpu()
    ref = torch.where(z >= 0, z, 0.1 * z)
    err = ((y.double() - ref).norm() / ref.norm()).item()
    assert err <= 1e-5, err


def test_x3_1x1_sliced_switch_selects_the_64_cout_kernel(shdr, monkeypatch):
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    shape = (1, 24, 24, 128, 0, 256, 1, False)
    tensors = _layer(shape, seed=5)

    def kernels():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            _run(K, shape, tensors)
        return {e.name for e in prof.events() if "conv_x3" in e.name}

    monkeypatch.delenv("SHDR_X3_1X1_SLICED", raising=False)
    new = kernels()
    monkeypatch.setenv("SHDR_X3_1X1_SLICED", "1")
    old = kernels()
    assert any("conv_x3_1x1_kernel" in k for k in new), new
    assert old and not any("conv_x3_1x1_kernel" in k for k in old), old
