"""conv_x3_kernel's issue order of the global loads (csrc/conv_x3.hip, template parameter LOOK: the filter unit of tap u + LOOK in front of
the chunk's patch loads, scalar-base filter loads by inline asm, counted vmcnt waits; SHDR_X3_LOOK=1|2) against the order of the first
rounds (SHDR_X3_LEGACY_PREFETCH=1): the same operands, the same MFMAs in the same order per accumulator and the same epilogue, so y, the
pooled output, the projected output and the output range slot are bit-identical.  A wrong wait count or slot shows as stale filter
registers in LDS, i.e. as different bits, at the smallest shapes that reach every path: 1, 2, 3 and 5 chunks (no prefetch; one; the
look-ahead running past the last unit), the chunk that crosses from the first source to the second, waves whose patch pieces lie
partly or wholly outside the image (the counted wait falls back), one and several cout slices, the phase loop of the stem."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SWITCH = "SHDR_X3_LOOK"                                       # the look-ahead of the new order
LEGACY = "SHDR_X3_LEGACY_PREFETCH"                            # =1: the order of the first rounds (LOOK = 0)
LOOKS = ["1", "2"]                                            # both look-aheads the nine-tap kernels are built with

# (N, H, W, C1, C2, Cout, epilogue)
CASES_3X3 = [
    (1, 16, 16, 32, 0, 64, "plain"), (1, 17, 19, 64, 0, 64, "plain"), (3, 5, 3, 96, 0, 128, "plain"), (1, 33, 47, 160, 0, 64, "plain"),
    (1, 17, 19, 32, 32, 64, "plain"), (3, 16, 16, 64, 32, 128, "plain"), (1, 33, 47, 32, 96, 32, "plain"), (1, 5, 3, 96, 0, 32, "plain"),
    (1, 17, 19, 64, 0, 64, "res"), (3, 16, 16, 160, 0, 128, "res"), (1, 33, 47, 32, 32, 64, "res"),
    (1, 16, 16, 64, 0, 64, "maxpool"), (2, 18, 22, 160, 0, 128, "maxpool"), (1, 16, 16, 96, 0, 64, "maxpool_only"),
    (1, 16, 16, 96, 0, 64, "avgpool"), (3, 16, 16, 32, 32, 64, "avgpool"),
    (1, 17, 19, 64, 0, 64, "proj"), (3, 16, 16, 160, 0, 64, "proj_maxpool"),
]
# (N, Hl, Wl, C, Cout, projected): the low-resolution input of the up-sampling prologue
CASES_UP = [(1, 8, 8, 32, 64, False), (1, 9, 11, 64, 128, False), (2, 1, 3, 96, 64, False), (3, 9, 11, 32, 128, False),
            (1, 9, 11, 96, 64, True), (1, 8, 8, 64, 64, True)]
CASES_STEM = [(1, 32, 32), (1, 33, 35), (2, 18, 16)]          # (N, H, W) of the 96-channel input of the 7x7 / stride-2 layer, Cout 64
CASES_1X1 = [(1, 17, 19, 64, 64), (1, 17, 19, 96, 64)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(new, old):
    assert len(new) == len(old) and len(new) > 0
    for a, b in zip(new, old):
        assert a.shape == b.shape
        assert torch.equal(_bits(a), _bits(b)), "%d of %d elements differ" % ((_bits(a) != _bits(b)).sum().item(), a.numel())


def _slot(K, t):
    s = K._range_of(t)
    assert s is not None
    return s.clone()


def _fresh(K, *ts):
    """clones with freshly measured range slots (an arm must not see a slot the other arm's launch wrote)"""
    out = []
    for t in ts:
        c = None if t is None else t.clone()
        if c is not None:
            K.absmax_slot(c)
        out.append(c)
    return out


def _arms(monkeypatch, run, look="1"):
    """run() under the new order (SHDR_X3_LOOK=look) and under the order of the first rounds: two lists of host tensors"""
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    res = []
    for new in (True, False):
        monkeypatch.setenv(SWITCH, look)
        if new:
            monkeypatch.delenv(LEGACY, raising=False)
        else:
            monkeypatch.setenv(LEGACY, "1")
        with torch.no_grad():
            out = run()
        torch.cuda.synchronize()
        res.append([t.cpu() for t in out])
    monkeypatch.delenv(LEGACY)
    return res


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _layer3(case, xscale=1.0, seed=None):
    n, h, w, c1, c2, cout, _ = case
    g = torch.Generator().manual_seed(sum(case[:6]) + 7 if seed is None else seed)
    x = _rand(g, n, h, w, c1, scale=xscale)
    x2 = _rand(g, n, h, w, c2, scale=xscale) if c2 else None
    wt = _rand(g, 3, 3, c1 + c2, cout, scale=1.0 / (3 * np.sqrt(c1 + c2)))
    b, sc, sh = _rand(g, cout), (torch.rand(cout, generator=g) + 0.5).cuda(), _rand(g, cout)
    res = _rand(g, n, h, w, cout)
    proj = _rand(g, 3, cout)
    return x, x2, wt, b, sc, sh, res, proj


def _run3(K, case, tensors, act1=None):
    n, h, w, c1, c2, cout, ep = case
    x, x2, wt, b, sc, sh, res, proj = tensors
    act1 = K.ACT_RELU if act1 is None else act1
    assert K.conv2d_plan((n, h, w, c1), tuple(wt.shape), c2=c2, has_residual=ep == "res") == "x3"
    xi, x2i = _fresh(K, x, x2)
    if ep == "plain":
        y = K.conv2d(xi, wt, b, x2=x2i, act1=act1)
        return [y, _slot(K, y)]
    if ep == "res":
        y = K.conv2d(xi, wt, b, x2=x2i, act1=act1, scale=sc, shift=sh, residual=res, act2=K.ACT_LRELU)
        return [y, _slot(K, y)]
    if ep == "maxpool":
        y, yp = K.conv2d_maxpool2(xi, wt, b, act1=act1)
        return [y, yp, _slot(K, yp)]
    if ep == "maxpool_only":
        yp = K.conv2d_maxpool2(xi, wt, b, act1=act1, keep_y=False)
        return [yp, _slot(K, yp)]
    if ep == "avgpool":
        y, yp = K.conv2d_avgpool2(xi, wt, b, act1=act1, x2=x2i)
        return [y, yp, _slot(K, yp)]
    if ep == "proj":
        yj = K._conv2d_raw(xi, wt, b, 1, None, 1.0, act1, None, None, None, K.ACT_NONE, K.ALGO_AUTO, None, None, None, None, 0, None, proj=proj)
        assert yj is not None
        return [yj]
    assert ep == "proj_maxpool"
    got = K.conv2d_maxpool2(xi, wt, b, act1=act1, proj=proj)
    assert got is not None
    return [got[0], got[1], _slot(K, got[1])]


@pytest.mark.parametrize("look", LOOKS)
@pytest.mark.parametrize("case", CASES_3X3)
def test_3x3_is_bit_identical(shdr, monkeypatch, case, look):
    K = shdr._ops
    tensors = _layer3(case)
    new, old = _arms(monkeypatch, lambda: _run3(K, case, tensors), look)
    _same(new, old)


def _layer_up(case, xscale=1.0):
    n, hl, wl, c, cout, _ = case
    g = torch.Generator().manual_seed(sum(case[:5]) + 11)
    return (_rand(g, n, hl, wl, c, scale=xscale), _rand(g, 3, 3, c, cout, scale=1.0 / (3 * np.sqrt(c))), _rand(g, cout),
            (torch.rand(cout, generator=g) + 0.5).cuda(), _rand(g, cout), _rand(g, 3, cout))


def _run_up(K, case, tensors):
    x, wt, b, sc, sh, proj = tensors
    (xi,) = _fresh(K, x)
    if case[5]:
        yj = K.conv2d_up2(xi, wt, b, act1=K.ACT_RELU, proj=proj)
        assert yj is not None
        return [yj]
    y = K.conv2d_up2(xi, wt, b, act1=K.ACT_RELU, scale=sc, shift=sh, act2=K.ACT_LRELU)
    return [y, _slot(K, y)]


@pytest.mark.parametrize("look", LOOKS)
@pytest.mark.parametrize("case", CASES_UP)
def test_up_is_bit_identical(shdr, monkeypatch, case, look):
    K = shdr._ops
    tensors = _layer_up(case)
    new, old = _arms(monkeypatch, lambda: _run_up(K, case, tensors), look)
    _same(new, old)


def _layer_stem(case):
    n, h, w = case
    g = torch.Generator().manual_seed(sum(case) + 13)
    return _rand(g, n, h, w, 96), _rand(g, 7, 7, 96, 64, scale=1.0 / (7 * np.sqrt(96))), _rand(g, 64)


def _run_stem(K, case, tensors):
    x, wt, b = tensors
    assert K.conv2d_plan(tuple(x.shape), tuple(wt.shape), stride=2) == "x3"
    (xi,) = _fresh(K, x)
    y = K.conv2d(xi, wt, b, stride=2, act1=K.ACT_RELU)
    return [y, _slot(K, y)]


@pytest.mark.parametrize("phase_launches", [False, True], ids=["one_launch", "phase_launches"])
@pytest.mark.parametrize("case", CASES_STEM)
def test_stem_is_bit_identical(shdr, monkeypatch, case, phase_launches):
    K = shdr._ops
    if phase_launches:
        monkeypatch.setenv("SHDR_X3_STEM_PHASE_LAUNCHES", "1")      # the 4x4, 4x3, 3x4 and 3x3 forms, partial sums in y
    tensors = _layer_stem(case)
    new, old = _arms(monkeypatch, lambda: _run_stem(K, case, tensors))
    _same(new, old)


def _run_1x1(K, tensors):
    x, wt, b = tensors
    assert K.conv2d_plan(tuple(x.shape), tuple(wt.shape)) == "x3"
    (xi,) = _fresh(K, x)
    y = K.conv2d(xi, wt, b, act1=K.ACT_RELU)
    return [y, _slot(K, y)]


@pytest.mark.parametrize("case", CASES_1X1)
def test_1x1_64_cout_form_is_bit_identical(shdr, monkeypatch, case):
    K = shdr._ops
    n, h, w, c, cout = case
    g = torch.Generator().manual_seed(sum(case) + 17)
    tensors = (_rand(g, n, h, w, c), _rand(g, 1, 1, c, cout, scale=1.0 / np.sqrt(c)), _rand(g, cout))
    new, old = _arms(monkeypatch, lambda: _run_1x1(K, tensors))
    _same(new, old)


def test_input_gradient_is_bit_identical(shdr, monkeypatch):
    """K.conv2d_dgrad of a 3x3 layer runs the transposed layer (128 -> 64 channels) on the same kernel"""
    K = shdr._ops
    g = torch.Generator().manual_seed(19)
    dz, wt = _rand(g, 1, 17, 19, 128, scale=1e-3), _rand(g, 3, 3, 64, 128, scale=0.04)
    names = set()

    def run():
        (dzi,) = _fresh(K, dz)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            dx = K.conv2d_dgrad(dzi, wt, (1, 17, 19, 64), 64, 0, 0)
            torch.cuda.synchronize()
        names.update(e.name for e in prof.events() if "conv_x3_kernel" in e.name)
        return [dx, _slot(K, dx)]

    new, old = _arms(monkeypatch, run)
    assert names, "the input gradient did not run conv_x3_kernel"
    _same(new, old)


@pytest.mark.parametrize("xscale", [1e5, 1e-7])
@pytest.mark.parametrize("case", [(1, 17, 19, 96, 0, 64, "plain"), (1, 33, 47, 32, 32, 64, "res")])
def test_3x3_is_bit_identical_at_range_ends(shdr, monkeypatch, case, xscale):
    K = shdr._ops
    tensors = _layer3(case, xscale=xscale)
    new, old = _arms(monkeypatch, lambda: _run3(K, case, tensors), "2")
    _same(new, old)


@pytest.mark.parametrize("xscale", [1e5, 1e-7])
@pytest.mark.parametrize("case", [(1, 9, 11, 64, 128, False), (2, 1, 3, 96, 64, False)])
def test_up_is_bit_identical_at_range_ends(shdr, monkeypatch, case, xscale):
    K = shdr._ops
    tensors = _layer_up(case, xscale=xscale)
    new, old = _arms(monkeypatch, lambda: _run_up(K, case, tensors), "2")
    _same(new, old)


def test_3x3_non_finite_inputs(shdr, monkeypatch):
    # no ReLU behind the convolution: it would turn the NaNs (inf - inf inside a dot product) into zeros
    K = shdr._ops
    case = (1, 17, 19, 96, 0, 64, "plain")
    tensors = list(_layer3(case))
    x = tensors[0].clone()
    x.view(-1)[::997] = float("inf")
    x.view(-1)[5::1013] = -float("inf")
    tensors[0] = x
    new, old = _arms(monkeypatch, lambda: _run3(K, case, tensors, act1=K.ACT_NONE))
    assert not torch.isfinite(new[0]).all()
    _same(new, old)                         # (NaNs included: the same bit patterns)


def _rel(y, ref):
    return ((y.double().cpu() - ref).norm() / ref.norm()).item()


def _conv_ref(x, wt, b, stride=1, pad=None):
    """float64 NHWC convolution on the host; pad = (top, bottom, left, right)"""
    xd = x.double().cpu().permute(0, 3, 1, 2)
    if pad is not None:
        xd = F.pad(xd, (pad[2], pad[3], pad[0], pad[1]))
    y = F.conv2d(xd, wt.double().cpu().permute(3, 2, 0, 1), b.double().cpu(), stride=stride, padding=0 if pad is not None else wt.shape[0] // 2)
    return y.permute(0, 2, 3, 1)


def test_3x3_vs_float64(shdr, monkeypatch):
    """the exact-fp32 bar of the split-operand kernels (1e-5) against a float64 reference, under the new order"""
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.setenv(SWITCH, "2")
    case = (2, 33, 47, 64, 32, 128, "plain")
    tensors = _layer3(case)
    x, x2, wt, b = tensors[:4]
    with torch.no_grad():
        y = _run3(K, case, tensors)[0]
    ref = torch.relu(_conv_ref(torch.cat([x, x2], dim=3), wt, b))
    err = _rel(y, ref)
    assert err <= 1e-5, err


def test_up_vs_float64(shdr, monkeypatch):
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.setenv(SWITCH, "1")
    case = (2, 9, 11, 96, 128, False)
    tensors = _layer_up(case)
    x, wt, b, sc, sh, _ = tensors
    with torch.no_grad():
        y = _run_up(K, case, tensors)[0]
    up = F.interpolate(x.double().cpu().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    z = torch.relu(_conv_ref(up, wt, b)) * sc.double().cpu() + sh.double().cpu()
    ref = torch.where(z >= 0, z, 0.1 * z)
    err = _rel(y, ref)
    assert err <= 1e-5, err


def test_stem_vs_float64(shdr, monkeypatch):
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    monkeypatch.setenv(SWITCH, "1")
    case = (2, 33, 35)
    tensors = _layer_stem(case)
    x, wt, b = tensors
    with torch.no_grad():
        y = _run_stem(K, case, tensors)[0]
    pads = []
    for size in (33, 35):                                       # TF SAME padding of a 7-tap / stride-2 filter
        total = max((-(-size // 2) - 1) * 2 + 7 - size, 0)
        pads += [total // 2, total - total // 2]
    ref = torch.relu(_conv_ref(x, wt, b, stride=2, pad=pads))
    assert tuple(ref.shape) == tuple(y.shape)
    err = _rel(y, ref)
    assert err <= 1e-5, err


def test_look_switch_selects_the_other_instantiation(shdr, monkeypatch):
    """the last template argument of conv_x3_kernel is the look-ahead: 2 on the nine-tap forms and 1 on the stem by default, 1 under
    SHDR_X3_LOOK=1, 0 under SHDR_X3_LEGACY_PREFETCH=1"""
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    case = (1, 17, 19, 64, 0, 64, "plain")
    tensors = _layer3(case)
    up_case = (1, 8, 8, 32, 64, False)
    up_tensors = _layer_up(up_case)
    stem_case = (1, 32, 32)
    stem_tensors = _layer_stem(stem_case)

    def looks():
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            with torch.no_grad():
                _run3(K, case, tensors)
                _run_up(K, up_case, up_tensors)
                _run_stem(K, stem_case, stem_tensors)
            torch.cuda.synchronize()
        found = {}
        for e in prof.events():
            m = re.search(r"conv_x3_kernel<(\w+), (\d+), (\d+), (\w+), (\d+)>", e.name)
            if m:
                found[m.group(1, 2, 3, 4)] = int(m.group(5))
        return found

    n33, up, stem = ("false", "3", "3", "false"), ("true", "3", "3", "false"), ("false", "4", "4", "true")
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv(LEGACY, raising=False)
    assert looks() == {n33: 2, up: 2, stem: 1}
    monkeypatch.setenv(SWITCH, "1")
    assert looks() == {n33: 1, up: 1, stem: 1}
    monkeypatch.setenv(LEGACY, "1")
    assert looks() == {n33: 0, up: 0, stem: 0}
