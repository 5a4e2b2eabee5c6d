"""conv_x3_kernel's issue order of the global loads (csrc/conv_x3.hip, template parameter LOOK: the filter unit of tap u + LOOK in front of
the chunk's patch loads, scalar-base filter loads by inline asm, counted vmcnt waits; SHDR_X3_LOOK=1|2) against the RECORDED output of
the order of the first rounds (LOOK = 0, removed: DESIGN.md section 6): the same operands, the same MFMAs in the same order per
accumulator and the same epilogue, so y, the pooled output, the projected output and the output range slot are bit-identical.  A wrong
wait count or slot shows as stale filter registers in LDS, i.e. as different bits, at the smallest shapes that reach every path: 1, 2, 3
and 5 chunks (no prefetch; one; the look-ahead running past the last unit), the chunk that crosses from the first source to the second,
waves whose patch pieces lie partly or wholly outside the image (the counted wait falls back), one and several cout slices, the phase
loop of the stem.

tests/golden/x3_prefetch_bits.json holds, per run of `entries()` below, the SHA-256 of every input tensor and the SHA-256 and shape of
every output.  It was written by tools/x3_bits_record.py from the last library that had the legacy order, under
SHDR_X3_LEGACY_PREFETCH=1, in the same session as that commit's version of this file, which compared the legacy arm with both
look-aheads live.  Record again only when a change alters the summation order on purpose."""
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SWITCH = "SHDR_X3_LOOK"                                       # the look-ahead
LOOKS = ["1", "2"]                                            # both look-aheads the nine-tap kernels are built with
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x3_prefetch_bits.json")

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
# (N, H, W) of the 96-channel input of the 7x7 / stride-2 layer, Cout 64; the last two: ragged tiles, odd output sizes
CASES_STEM = [(1, 32, 32), (1, 33, 35), (2, 18, 16), (1, 64, 80), (2, 70, 46)]
CASES_1X1 = [(1, 17, 19, 64, 64), (1, 17, 19, 96, 64)]
CASES_3X3_ENDS = [(1, 17, 19, 96, 0, 64, "plain"), (1, 33, 47, 32, 32, 64, "res")]
CASES_UP_ENDS = [(1, 9, 11, 64, 128, False), (2, 1, 3, 96, 64, False)]
RANGE_ENDS = [1e5, 1e-7]
CASE_NON_FINITE = (1, 17, 19, 96, 0, 64, "plain")
# the outputs of a run by name, in the order the runners below return them
NAMES_3X3 = {"plain": ("y", "range"), "res": ("y", "range"), "maxpool": ("y", "pooled", "range"), "maxpool_only": ("pooled", "range"),
             "avgpool": ("y", "pooled", "range"), "proj": ("projected",), "proj_maxpool": ("projected", "pooled", "range")}
NAMES_UP = {False: ("y", "range"), True: ("projected",)}


def _slot(K, t):
    s = K._range_of(t)
    assert s is not None
    return s.clone()


def _fresh(K, *ts):
    """clones with freshly measured range slots (a run must not see a slot an earlier launch wrote)"""
    out = []
    for t in ts:
        c = None if t is None else t.clone()
        if c is not None:
            K.absmax_slot(c)
        out.append(c)
    return out


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["runs"]


def _check(K, monkeypatch, key, looks):
    """the run `key` of entries() under every look-ahead of `looks` against its record; returns the outputs of the last run by name"""
    tensors, run, names = entries(K)[key]()
    want = _golden()[key]
    got_in = [digest(t) for t in tensors if t is not None]
    assert got_in == want["inputs"], "%s: the seeded inputs are not the recorded ones (torch's generator changed?): re-record %s with " \
        "tools/x3_bits_record.py" % (key, os.path.basename(GOLDEN))
    assert [o["name"] for o in want["outputs"]] == list(names)
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    out = None
    for look in looks:
        monkeypatch.setenv(SWITCH, look)
        with torch.no_grad():
            out = run()
        torch.cuda.synchronize()
        assert len(out) == len(names)
        for name, t, w in zip(names, out, want["outputs"]):
            assert list(t.shape) == w["shape"], "%s, %s=%s: %s has shape %s, recorded %s" % (key, SWITCH, look, name, list(t.shape), w["shape"])
            assert digest(t) == w["sha256"], "%s, %s=%s: the bits of %s differ from the recorded ones" % (key, SWITCH, look, name)
    return dict(zip(names, out))


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


def _run_1x1(K, tensors):
    x, wt, b = tensors
    assert K.conv2d_plan(tuple(x.shape), tuple(wt.shape)) == "x3"
    (xi,) = _fresh(K, x)
    y = K.conv2d(xi, wt, b, act1=K.ACT_RELU)
    return [y, _slot(K, y)]


def _layer_1x1(case):
    n, h, w, c, cout = case
    g = torch.Generator().manual_seed(sum(case) + 17)
    return _rand(g, n, h, w, c), _rand(g, 1, 1, c, cout, scale=1.0 / np.sqrt(c)), _rand(g, cout)


def _layer_dgrad():
    g = torch.Generator().manual_seed(19)
    return _rand(g, 1, 17, 19, 128, scale=1e-3), _rand(g, 3, 3, 64, 128, scale=0.04)


def _run_dgrad(K, tensors, names=None):
    """K.conv2d_dgrad of a 3x3 layer runs the transposed layer (128 -> 64 channels) on the same kernel; names: the kernels it ran"""
    dz, wt = tensors
    (dzi,) = _fresh(K, dz)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        dx = K.conv2d_dgrad(dzi, wt, (1, 17, 19, 64), 64, 0, 0)
        torch.cuda.synchronize()
    if names is not None:
        names.update(e.name for e in prof.events() if "conv_x3_kernel" in e.name)
    return [dx, _slot(K, dx)]


def _layer_non_finite():
    tensors = list(_layer3(CASE_NON_FINITE))
    x = tensors[0].clone()
    x.view(-1)[::997] = float("inf")
    x.view(-1)[5::1013] = -float("inf")
    tensors[0] = x
    return tensors


DGRAD_KERNELS = set()                                         # filled by the input-gradient run


def entries(K):
    """key -> builder of (input tensors, run, output names) for every recorded run: the tests look themselves up here and
    tools/x3_bits_record.py walks all of it.  run() returns the outputs in the order of the names."""
    e = {}

    def add(key, layer, run, names):
        def build():
            tensors = layer()
            return tensors, (lambda: run(tensors)), names
        assert key not in e
        e[key] = build

    for c in CASES_3X3:
        add("3x3 %r" % (c,), lambda c=c: _layer3(c), lambda t, c=c: _run3(K, c, t), NAMES_3X3[c[6]])
    for c in CASES_UP:
        add("up %r" % (c,), lambda c=c: _layer_up(c), lambda t, c=c: _run_up(K, c, t), NAMES_UP[c[5]])
    for c in CASES_STEM:
        add("stem %r" % (c,), lambda c=c: _layer_stem(c), lambda t, c=c: _run_stem(K, c, t), ("y", "range"))
    for c in CASES_1X1:
        add("1x1 %r" % (c,), lambda c=c: _layer_1x1(c), lambda t: _run_1x1(K, t), ("y", "range"))
    add("dgrad", _layer_dgrad, lambda t: _run_dgrad(K, t, DGRAD_KERNELS), ("dx", "range"))
    for xs in RANGE_ENDS:
        for c in CASES_3X3_ENDS:
            add("3x3 %r x %g" % (c, xs), lambda c=c, xs=xs: _layer3(c, xscale=xs), lambda t, c=c: _run3(K, c, t), NAMES_3X3[c[6]])
        for c in CASES_UP_ENDS:
            add("up %r x %g" % (c, xs), lambda c=c, xs=xs: _layer_up(c, xscale=xs), lambda t, c=c: _run_up(K, c, t), NAMES_UP[c[5]])
    # no ReLU behind the convolution: it would turn the NaNs (inf - inf inside a dot product) into zeros
    add("3x3 non-finite", _layer_non_finite, lambda t: _run3(K, CASE_NON_FINITE, t, act1=K.ACT_NONE), NAMES_3X3["plain"])
    return e


@pytest.mark.parametrize("look", LOOKS)
@pytest.mark.parametrize("case", CASES_3X3)
def test_3x3_is_bit_identical(shdr, monkeypatch, case, look):
    _check(shdr._ops, monkeypatch, "3x3 %r" % (case,), [look])


@pytest.mark.parametrize("look", LOOKS)
@pytest.mark.parametrize("case", CASES_UP)
def test_up_is_bit_identical(shdr, monkeypatch, case, look):
    _check(shdr._ops, monkeypatch, "up %r" % (case,), [look])


@pytest.mark.parametrize("case", CASES_STEM)
def test_stem_is_bit_identical(shdr, monkeypatch, case):
    _check(shdr._ops, monkeypatch, "stem %r" % (case,), ["1"])


@pytest.mark.parametrize("case", CASES_1X1)
def test_1x1_64_cout_form_is_bit_identical(shdr, monkeypatch, case):
    _check(shdr._ops, monkeypatch, "1x1 %r" % (case,), ["1"])


def test_input_gradient_is_bit_identical(shdr, monkeypatch):
    DGRAD_KERNELS.clear()
    _check(shdr._ops, monkeypatch, "dgrad", ["1"])
    assert DGRAD_KERNELS, "the input gradient did not run conv_x3_kernel"


@pytest.mark.parametrize("xscale", RANGE_ENDS)
@pytest.mark.parametrize("case", CASES_3X3_ENDS)
def test_3x3_is_bit_identical_at_range_ends(shdr, monkeypatch, case, xscale):
    _check(shdr._ops, monkeypatch, "3x3 %r x %g" % (case, xscale), ["2"])


@pytest.mark.parametrize("xscale", RANGE_ENDS)
@pytest.mark.parametrize("case", CASES_UP_ENDS)
def test_up_is_bit_identical_at_range_ends(shdr, monkeypatch, case, xscale):
    _check(shdr._ops, monkeypatch, "up %r x %g" % (case, xscale), ["2"])


def test_3x3_non_finite_inputs(shdr, monkeypatch):
    out = _check(shdr._ops, monkeypatch, "3x3 non-finite", ["1"])
    assert not torch.isfinite(out["y"]).all()                 # (NaNs included in the record: the same bit patterns)


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
    SHDR_X3_LOOK=1"""
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
    assert looks() == {n33: 2, up: 2, stem: 1}
    monkeypatch.setenv(SWITCH, "1")
    assert looks() == {n33: 1, up: 1, stem: 1}
