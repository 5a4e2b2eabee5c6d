"""The NHWC pooling / resize / global-average-pool kernels and the BatchNorm finalisers (csrc/nhwc_vec.h, instantiated for fp32 by
csrc/pool.hip and csrc/bwd.hip and for fp16 by csrc/elem_f16.hip) against the RECORDED bits of the library that still had one hand-written
copy per precision.  The exact tests of test_gpu_tape_f32.py and test_gpu_fp16_elem.py use integer-valued inputs, for which every
summation order and every contraction give the same result: they cannot see a changed association or a lost or gained FMA.  Here the
inputs are seeded normal values of scale 1 without any structure, and the assertion is equality of SHA-256 digests.

tests/golden/nhwc_family_bits.json holds, per run of `entries()` below, the SHA-256 of every input tensor and the SHA-256 and shape of
every output (the range slot of the fp32 resize2x_bwd, mean / var / moving statistics / dgamma / dbeta of BatchNorm included).  It was
written by tools/nhwc_bits_record.py on an MI355X from a build of the commit named in the file, twice, with identical digests.  Record
again only when a change alters the arithmetic of one of these kernels on purpose.

Shapes per operation: (2, 5, 7, C) with C = 12 (fp32) / 24 (fp16) -- odd sizes, three vectors per pixel, (2, 6, 8, C) for the even-only
maxpool2; one vector (1, 1, 1, C) where the operation allows H = W = 1; a loop domain just past the 2048 x 256 threads of
shdr::stream_grid (the GS of the two per-element test files); for gap also HW = 63 and HW = 260 (the four-in-flight loop and its tail)."""
import hashlib
import json
import os
import zlib

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nhwc_family_bits.json")
GS = {False: (1, 132, 256, 64), True: (1, 264, 256, 64)}      # fp32 / fp16: 540 672 16-byte vectors
EPS = 1e-3


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def _t(g, shape, h):
    t = torch.randn(*shape, generator=g)
    return (t.half() if h else t).cuda()


def _f(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def _half(s):
    return (s[0], s[1] // 2, s[2] // 2, s[3])


def _ceil_half(s):
    return (s[0], (s[1] + 1) // 2, (s[2] + 1) // 2, s[3])


def _double(s):
    return (s[0], 2 * s[1], 2 * s[2], s[3])


def _fwd(K, op, key, shape, h):
    x = _t(_gen(key), shape, h)
    return [x], lambda: (getattr(K, op)(x),), ("y",)


def _avgpool2_bwd(K, key, shape, h):
    dy = _t(_gen(key), _half(shape), h)
    return [dy], lambda: (K.avgpool2_bwd(dy, shape),), ("dx",)


def _maxpool2_bwd(K, key, shape, h):
    g = _gen(key)
    x, dy = _t(g, shape, h), _t(g, _half(shape), h)
    return [x, dy], lambda: (K.maxpool2_bwd(x, dy),), ("dx",)


def _maxpool3s2_bwd(K, key, shape, h):
    g = _gen(key)
    x = _t(g, shape, h)
    y = K.maxpool3s2(x)                                        # the pooled output is an operand of the backward
    dy = _t(g, tuple(y.shape), h)
    return [x, y, dy], lambda: (K.maxpool3s2_bwd(x, y, dy),), ("dx",)


def _resize2x_bwd(K, key, shape, h):
    dy = _t(_gen(key), _double(shape), h)

    def run():
        dx = K.resize2x_bwd(dy, shape)
        return (dx,) if h else (dx, K._range_of(dx).clone())
    return [dy], run, ("dx",) if h else ("dx", "range")


def _upsample_zero2(K, key, shape, h):
    dy = _t(_gen(key), _ceil_half(shape), h)
    return [dy], lambda: (K.upsample_zero2(dy, shape),), ("dx",)


def _gap_bwd(K, key, shape, h):
    dy = _f(_gen(key), shape[0], shape[3])
    return [dy], lambda: (K.gap_bwd(dy, shape, dtype=torch.float16 if h else torch.float32),), ("dx",)


def _bn_stats(K, key, shape, h):
    g = _gen(key)
    x, mm, mv = _t(g, shape, h), _f(g, shape[3]), _f(g, shape[3]).abs() + 0.5

    def run():
        m, v = mm.clone(), mv.clone()
        mean, var = K.bn_stats(x, m, v, 0.99)
        return mean, var, m, v
    return [x, mm, mv], run, ("mean", "var", "moving_mean", "moving_var")


def _bn_bwd(K, key, shape, h):
    g = _gen(key)
    c = shape[3]
    dy, x, y_relu = _t(g, shape, h), _t(g, shape, h), _t(g, shape, h)
    gamma, dg0, db0 = _f(g, c), _f(g, c), _f(g, c)
    mean, var = K.bn_stats(x)

    def run():
        dg, db = dg0.clone(), db0.clone()
        dx, dg, db = K.bn_bwd(dy, x, y_relu, mean, var, gamma, EPS, dg, db)
        return dx, dg, db
    return [dy, x, y_relu, gamma, dg0, db0, mean, var], run, ("dx", "dgamma", "dbeta")


def entries(K):
    """key -> builder of (input tensors, run() -> outputs, output names)"""
    E = {}
    for h in (False, True):
        c = 24 if h else 12
        small, even, one, gs = (2, 5, 7, c), (2, 6, 8, c), (1, 1, 1, c // 3), GS[h]
        big = _double(gs)                                      # the input of an op whose loop runs over its half-size output

        def add(op, shape, build, *args, h=h):
            key = "%s_%s_%s" % (op, "f16" if h else "f32", "x".join(str(d) for d in shape))
            E[key] = lambda: build(K, *args, key, shape, h)

        for s in (small, big):
            add("avgpool2", s, _fwd, "avgpool2")
        for s in (even, big):
            add("maxpool2", s, _fwd, "maxpool2")
            add("maxpool2_bwd", s, _maxpool2_bwd)
        for s in (small, gs):
            add("avgpool2_bwd", s, _avgpool2_bwd)
        for s in (small, one, big):
            add("maxpool3s2", s, _fwd, "maxpool3s2")
        for s in (small, one, gs):
            add("maxpool3s2_bwd", s, _maxpool3s2_bwd)
            add("resize2x", s, _fwd, "resize2x")
            add("resize2x_bwd", s, _resize2x_bwd)
            add("upsample_zero2", s, _upsample_zero2)
            add("gap_bwd", s, _gap_bwd)
            add("bn_stats", s, _bn_stats)
            add("bn_bwd", s, _bn_bwd)
        for s in (small, one, gs, (2, 7, 9, c), (2, 13, 20, c)):
            add("gap", s, _fwd, "global_avg_pool")
    return E


KEYS = sorted(entries(None))


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_file_holds_every_entry(golden):
    assert sorted(golden["runs"]) == KEYS
    assert len(golden["commit"]) == 40


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_bits_as_recorded(K, golden, key):
    tensors, run, names = entries(K)[key]()
    want = golden["runs"][key]
    assert [digest(t) for t in tensors] == want["inputs"], "%s: the inputs are not the recorded ones (torch's generator changed, or a " \
        "kernel that prepares an operand): re-record %s with tools/nhwc_bits_record.py" % (key, os.path.basename(GOLDEN))
    assert [o["name"] for o in want["outputs"]] == list(names)
    with torch.no_grad():
        out = run()
    torch.cuda.synchronize()
    assert len(out) == len(names)
    for name, t, w in zip(names, out, want["outputs"]):
        assert list(t.shape) == w["shape"], "%s: %s has shape %s, recorded %s" % (key, name, list(t.shape), w["shape"])
        assert digest(t) == w["sha256"], "%s: the bits of %s differ from the recorded ones" % (key, name)
