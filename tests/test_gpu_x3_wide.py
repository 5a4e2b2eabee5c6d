"""The 128-cout 3x3 split-operand kernel (conv_x3_wide_kernel<UP>, csrc/conv_x3.hip), plain and with the bilinear 2x prologue, against the
64-cout kernel it replaces (SHDR_X3_SLICED=1): the same operands, chunk and tap order, MFMA order and epilogue, so y, the pooled output and the output
range slot are bit-identical.  The shapes are the smallest at which the new parts can go wrong: one chunk (no prefetch), two, five
(odd: the parity of the double-buffered patch), two sources, sizes off the 16-pixel tile, one to three 128-cout blocks per pixel tile.
The switches SHDR_X3_WIDE_MIN_BLOCKS=1 and SHDR_X3_WIDE_MIN_COUT=128 take the dispatch thresholds (speed only) out of the way."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, H, W, C1, C2, Cout, residual + affine map + second activation)
SHAPES = [
    (1, 1, 3, 32, 0, 128, False), (2, 17, 19, 64, 0, 128, True), (3, 33, 31, 160, 0, 256, False), (1, 17, 19, 64, 32, 384, True),
    (1, 17, 19, 64, 32, 256, False), (1, 33, 31, 160, 0, 128, True), (2, 1, 3, 64, 0, 256, True), (1, 17, 19, 160, 0, 384, False),
    (3, 17, 19, 32, 0, 256, True), (2, 33, 31, 64, 32, 128, False),
    # Cout 192 is no multiple of 128: it stays on the 64-cout kernel, the result is the same
    (2, 33, 31, 32, 0, 192, False), (1, 17, 19, 64, 32, 192, True),
]
POOLED = [(1, 18, 20, 64, 0, 128), (2, 34, 30, 160, 0, 256), (1, 34, 30, 32, 0, 384), (3, 18, 20, 64, 32, 128)]


def _layer(shape, seed, xscale=1.0, special=False):
    n, h, w, c1, c2, cout, has_res = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c1, generator=g) * xscale
    x2 = torch.randn(n, h, w, c2, generator=g) * 255.0 * xscale if c2 else None
    if special:
        x.view(-1)[::997] = float("inf")
        x.view(-1)[5::1013] = -float("inf")
    wt = torch.randn(3, 3, c1 + c2, cout, generator=g) / (3 * np.sqrt(c1 + c2))
    b, sc, sh = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    res = torch.randn(n, h, w, cout, generator=g) if has_res else None
    return [None if t is None else t.cuda() for t in (x, x2, wt, b, sc, sh, res)]


def _slot(K, y):
    slot = K._range_of(y)
    assert slot is not None
    return slot.cpu().view(torch.int32).clone()


def _run(K, shape, tensors, act1=None, pool=None):
    n, h, w, c1, c2, cout, has_res = shape
    x, x2, wt, b, sc, sh, res = tensors
    x2s = 1.0 / 255 if c2 else 1.0
    assert K.conv2d_plan((n, h, w, c1), tuple(wt.shape), c2=c2, x2_scale=x2s, has_residual=has_res) == "x3"
    act1 = K.ACT_RELU if act1 is None else act1
    with torch.no_grad():
        xi, x2i = x.clone(), None if x2 is None else x2.clone()      # fresh tensors: fresh range slots
        K.absmax_slot(xi)
        if x2i is not None:
            K.absmax_slot(x2i)
        if pool == "max":
            y, yp = K.conv2d_maxpool2(xi, wt, b, act1=act1)
        elif pool == "avg":
            y, yp = K.conv2d_avgpool2(xi, wt, b, act1=act1, x2=x2i)
        else:
            yp = None
            if has_res:
                y = K.conv2d(xi, wt, b, x2=x2i, x2_scale=x2s, act1=act1, scale=sc, shift=sh, residual=res, act2=K.ACT_LRELU)
            else:
                y = K.conv2d(xi, wt, b, x2=x2i, x2_scale=x2s, act1=act1)
    torch.cuda.synchronize()
    return y.cpu(), _slot(K, y), None if yp is None else yp.cpu()


def _both(shdr, monkeypatch, shape, act1=None, pool=None, **kw):
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_COUT", "128")
    tensors = _layer(shape, seed=sum(shape[:6]) + 3, **kw)
    monkeypatch.delenv("SHDR_X3_SLICED", raising=False)
    new = _run(K, shape, tensors, act1, pool)
    monkeypatch.setenv("SHDR_X3_SLICED", "1")
    old = _run(K, shape, tensors, act1, pool)
    monkeypatch.delenv("SHDR_X3_SLICED")
    return new, old


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("shape", SHAPES)
def test_x3_wide_block_is_bit_identical(shdr, monkeypatch, shape):
    (y1, r1, _), (y0, r0, _) = _both(shdr, monkeypatch, shape)
    assert _bits_equal(y1, y0), "max |diff| %g" % (y1 - y0).abs().max().item()
    assert torch.equal(r1, r0)


@pytest.mark.parametrize("pool", ["max", "avg"])
@pytest.mark.parametrize("shape", POOLED)
def test_x3_wide_block_pooled_output_is_bit_identical(shdr, monkeypatch, shape, pool):
    if pool == "max" and shape[4]:
        shape = shape[:4] + (0,) + shape[5:]                 # (the max-pooled form takes one source)
    (y1, r1, p1), (y0, r0, p0) = _both(shdr, monkeypatch, shape + (False,), pool=pool)
    assert _bits_equal(y1, y0)
    assert _bits_equal(p1, p0)
    assert torch.equal(r1, r0)


@pytest.mark.parametrize("xscale", [1e5, 1e-7])
@pytest.mark.parametrize("shape", [(1, 33, 31, 64, 32, 256, True), (2, 17, 19, 160, 0, 128, False)])
def test_x3_wide_block_is_bit_identical_at_range_ends(shdr, monkeypatch, shape, xscale):
    (y1, r1, _), (y0, r0, _) = _both(shdr, monkeypatch, shape, xscale=xscale)
    assert _bits_equal(y1, y0)
    assert torch.equal(r1, r0)


def test_x3_wide_block_non_finite_inputs(shdr, monkeypatch):
    # no ReLU in front of the affine map: it would turn the NaNs (inf - inf inside a dot product) into zeros
    (y1, r1, _), (y0, r0, _) = _both(shdr, monkeypatch, (1, 21, 23, 64, 32, 256, True), act1=shdr._ops.ACT_NONE, special=True)
    assert not torch.isfinite(y1).all()
    assert _bits_equal(y1, y0)              # (NaNs included: the same bit patterns)
    assert torch.equal(r1, r0)


def test_x3_wide_block_vs_float64(shdr, monkeypatch):
    """the exact-fp32 bar of the split-operand kernels (1e-5) against a float64 reference"""
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_COUT", "128")
    shape = (2, 33, 29, 64, 32, 256, True)
    x, x2, wt, b, sc, sh, res = _layer(shape, seed=11)
    y, _, _ = _run(K, shape, (x, x2, wt, b, sc, sh, res))
    xd = torch.cat([x.double(), x2.double() / 255.0], dim=3).cpu().permute(0, 3, 1, 2)
    z = torch.nn.functional.conv2d(xd, wt.double().cpu().permute(3, 2, 0, 1), b.double().cpu(), padding=1).permute(0, 2, 3, 1)
    z = torch.relu(z) * sc.double().cpu() + sh.double().cpu() + res.double().cpu()
    ref = torch.where(z >= 0, z, 0.1 * z)
    err = ((y.double() - ref).norm() / ref.norm()).item()
    assert err <= 1e-5, err


def test_x3_sliced_switch_selects_the_64_cout_kernel(shdr, monkeypatch):
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_COUT", "128")
    shape = (1, 24, 24, 64, 0, 256, False)
    tensors = _layer(shape, seed=5)

    def kernels():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            _run(K, shape, tensors)
        return {e.name for e in prof.events() if "conv_x3" in e.name}

    monkeypatch.delenv("SHDR_X3_SLICED", raising=False)
    new = kernels()
    monkeypatch.setenv("SHDR_X3_SLICED", "1")
    old = kernels()
    assert any("conv_x3_wide_kernel<false>" in k for k in new), new
    assert old and not any("conv_x3_wide_kernel" in k for k in old), old


def test_x3_wide_block_default_threshold_runs_the_wide_kernel_on_a_full_grid(shdr, monkeypatch):
    """without the test switches: a 512-cout layer with 256 blocks of 128 couts goes wide, a smaller or narrower one does not"""
    K = shdr._ops

    def kernels(shape):
        tensors = _layer(shape, seed=7)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            _run(K, shape, tensors)
        return {e.name for e in prof.events() if "conv_x3" in e.name}

    big = kernels((1, 128, 128, 32, 0, 512, False))          # 64 tiles x 4 = 256 wide blocks
    small = kernels((1, 64, 128, 32, 0, 512, False))         # 128 wide blocks (256 of the 64-cout kernel: still plan x3)
    assert any("conv_x3_wide_kernel" in k for k in big), big
    narrow = kernels((1, 128, 256, 32, 0, 256, False))      # 256 wide blocks, but 256 couts
    assert small and not any("conv_x3_wide_kernel" in k for k in small), small
    assert narrow and not any("conv_x3_wide_kernel" in k for k in narrow), narrow


# ---- the bilinear 2x prologue (conv_x3_wide_kernel<true>): (N, low-res H, W, C, Cout) -------------------------------------------------
UP_SHAPES = [(1, 1, 2, 32, 128), (2, 9, 10, 64, 128), (1, 17, 15, 160, 128), (3, 1, 2, 64, 256), (1, 9, 10, 160, 256), (2, 17, 15, 32, 256)]


def _layer_up(shape, seed):
    n, hl, wl, c, cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hl, wl, c, generator=g)
    wt = torch.randn(3, 3, c, cout, generator=g) / (3 * np.sqrt(c))
    b, sc, sh = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    return [t.cuda() for t in (x, wt, b, sc, sh)]


def _run_up(K, tensors, two_kernels=False):
    x, wt, b, sc, sh = tensors
    with torch.no_grad():
        xi = x.clone()
        K.absmax_slot(xi)
        if two_kernels:
            y = K.conv2d(K.resize2x(xi), wt, b, act1=K.ACT_RELU, scale=sc, shift=sh, act2=K.ACT_LRELU)
        else:
            y = K.conv2d_up2(xi, wt, b, act1=K.ACT_RELU, scale=sc, shift=sh, act2=K.ACT_LRELU)
    torch.cuda.synchronize()
    return y.cpu(), _slot(K, y)


def _switches(monkeypatch):
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_BLOCKS", "1")
    monkeypatch.setenv("SHDR_X3_WIDE_MIN_COUT", "128")
    monkeypatch.delenv("SHDR_X3_SLICED", raising=False)


@pytest.mark.parametrize("shape", UP_SHAPES)
def test_x3_wide_block_bilinear_prologue_is_bit_identical(shdr, monkeypatch, shape):
    K = shdr._ops
    _switches(monkeypatch)
    tensors = _layer_up(shape, seed=sum(shape) + 17)
    y1, r1 = _run_up(K, tensors)
    monkeypatch.setenv("SHDR_X3_SLICED", "1")
    y0, r0 = _run_up(K, tensors)
    assert _bits_equal(y1, y0), "max |diff| %g" % (y1 - y0).abs().max().item()
    assert torch.equal(r1, r0)


def test_x3_wide_block_bilinear_prologue_matches_resize_and_plain(shdr, monkeypatch):
    K = shdr._ops
    _switches(monkeypatch)
    tensors = _layer_up((2, 17, 15, 64, 256), seed=23)
    y1, _ = _run_up(K, tensors)
    monkeypatch.setenv("SHDR_X3_SLICED", "1")
    y0, _ = _run_up(K, tensors, two_kernels=True)
    assert _bits_equal(y1, y0), "max |diff| %g" % (y1 - y0).abs().max().item()


def test_x3_sliced_switch_selects_the_64_cout_kernel_bilinear_prologue(shdr, monkeypatch):
    K = shdr._ops
    _switches(monkeypatch)
    tensors = _layer_up((1, 12, 12, 64, 256), seed=5)

    def kernels():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            _run_up(K, tensors)
        return {e.name for e in prof.events() if "conv_x3" in e.name}

    new = kernels()
    monkeypatch.setenv("SHDR_X3_SLICED", "1")
    old = kernels()
    assert any("conv_x3_wide_kernel<true>" in k for k in new), new
    assert old and all("conv_x3_kernel<true" in k for k in old), old
