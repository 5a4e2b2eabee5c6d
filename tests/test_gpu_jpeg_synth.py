"""The device JPEG decoder (csrc/jpeg.hip, singlehdr-tf2_amd/jpeg.py) on the files of tests/jpeg_synth.py: streams built
coefficient by coefficient, so the expected coefficients are the writer's input and the expected pixels are PIL's
(tests/test_jpeg_synth.py proves on the host that the reference agrees with both).  They pin what PIL-written files never
reach: Huffman tables whose codes are all longer than the 9-bit look-ahead, a 9/10-bit boundary inside a table, one-symbol
tables, four table slots in one scan, DC differences of category 11, AC values of category 10, ZRL ZRL ZRL + run 14 up to zig-zag
63, blocks without EOB, chroma planes 2 and 3 wide, and streams of zero bits that never re-synchronise: there the
Weissenberger-Schmidt scheme degenerates to its sequential chain, one pass per workgroup, and the pass counts and rounds must be
those of jpeg_synth.sync_model."""
import struct

import numpy as np
import pytest
import torch

import jpeg_ref
import jpeg_synth
from jpeg_synth import CASES

pytestmark = pytest.mark.gpu

ACCEPTED = [c for c in CASES if c.refused is None]
SMALL = [c for c in ACCEPTED if c.small]
MULTI = [c for c in ACCEPTED if c.multi]                                  # the stream-shape cases and the 16-bit-code tables
BY_NAME = {c.name: c for c in CASES}
ROUND = jpeg_synth.WG + 2                                                  # sync_rounds: pass * (WG + 2) + iteration
ids = lambda cases: [c.name for c in cases]


@pytest.fixture(scope="module")
def jpeg(shdr):
    return shdr.jpeg


def _assert_coefficients(got, want, name):
    assert len(got) == len(want), name
    for c, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == torch.int16 and tuple(a.shape) == b.shape, (name, c)
        assert np.array_equal(a.cpu().numpy(), b), (name, c)


@pytest.fixture(scope="module")
def singles(jpeg):
    """every small case decoded on its own, once: {name: (coefficients per component, pixels)} as host arrays"""
    out = {}
    for c in SMALL:
        d = jpeg.Decoded([c.data])
        out[c.name] = ([a.cpu().numpy() for a in d.coefficients(0)], d.image(0).cpu().numpy(), d.errors.cpu().tolist())
    return out


@pytest.mark.parametrize("case", ACCEPTED, ids=ids(ACCEPTED))
def test_coefficients_are_the_writers_input_and_pixels_pils(jpeg, case):
    _assert_coefficients(jpeg.decode_coefficients(case.data), case.coef, case.name)
    if not case.pixels:                                                    # the two extreme cases: coefficients and a clean error word
        assert case.name in jpeg_synth.EXTREME
        d = jpeg.Decoded([case.data], pixels=False)
        assert d.errors.cpu().tolist() == [0]
        return
    rgb = jpeg.decode([case.data])[0]
    assert rgb.dtype == torch.uint8 and rgb.is_cuda and tuple(rgb.shape) == case.pil.shape, case.name
    assert np.array_equal(rgb.cpu().numpy(), case.pil), case.name


@pytest.mark.parametrize("bits", [256, 512, 1024, 2048])
@pytest.mark.parametrize("case", MULTI, ids=ids(MULTI))
def test_every_subsequence_length_on_stream_shapes(jpeg, case, bits):
    d = jpeg.Decoded([case.data], subseq_bits=bits)
    d.check()
    assert d.errors.cpu().tolist() == [0]
    _assert_coefficients(d.coefficients(0), case.coef, case.name)
    assert np.array_equal(d.image(0).cpu().numpy(), case.pil), case.name
    valid = d.plan.sub_seg >= 0
    n_wg = int(d.plan.images["n_wg"][0])
    rounds = d.sync_rounds()
    assert rounds.shape == valid.shape and np.all(rounds[valid] >= 0) and np.all(rounds[~valid] == -1)
    # the last change lies in the last pass or, where that pass only confirmed, in the one before
    assert max(d.passes - 2, 0) <= int(rounds.max()) // ROUND <= d.passes - 1, (d.passes, int(rounds.max()))
    print("\n%s at %d bits: %d workgroups, %d passes, last change in round %d" % (case.name, bits, n_wg, d.passes, rounds.max()), end="")
    if case.zero_stream:
        # no subsequence re-synchronises: whatever the model says, a workgroup cannot be final before its left neighbour is
        assert d.passes >= max(2, n_wg)
        if bits <= 512:
            assert d.passes >= 3
        if bits == 256:
            assert d.passes >= 5
        a = case.args
        mx, my, _ = jpeg_synth.block_grid(a["width"], a["height"], a["comps"])
        model = jpeg_synth.sync_model(case.zero_stream, mx * my, bits, detail=True)
        print(" (model: %d workgroups, %d passes, iterations %s, last change in round %d)" % (
            model.workgroups, model.passes, model.iterations, model.rounds.max()), end="")
        assert n_wg == model.workgroups and d.passes == model.passes
        assert int(rounds.max()) // ROUND == (d.passes - 1 if n_wg > 1 else 0)
        assert np.array_equal(rounds, model.rounds)
    if case.name.startswith("noise") and bits == 256:
        by_wg = d.plan.sub_seg.reshape(-1, jpeg.WG)
        assert any(wg > 0 and by_wg[wg, 0] == by_wg[wg - 1, -1] for wg in range(by_wg.shape[0]))      # starts inside a segment
        assert any(len(set(row[row >= 0].tolist())) >= 2 for row in by_wg)                              # holds two segments
    again = jpeg.Decoded([case.data], subseq_bits=bits)
    assert again.passes == d.passes and torch.equal(again.out, d.out) and torch.equal(again.coef, d.coef)


def _batch_items():
    half = len(SMALL) // 2
    return SMALL[:half] + [BY_NAME["zeros-422"]] + SMALL[half:]


@pytest.fixture(scope="module")
def batch(jpeg):
    cases = _batch_items()
    return cases, jpeg.Decoded([c.data for c in cases])


def test_batch_of_more_than_64_images(jpeg, batch, singles):
    """every small case and, in the middle, a stream that needs a pass per workgroup: each image as if decoded alone"""
    cases, d = batch
    assert len(cases) > 64 + 1 and d.errors.cpu().tolist() == [0] * len(cases)
    assert d.passes >= 3                                                   # zeros-422 at the default 512 bits: three workgroups
    for i, c in enumerate(cases):
        if c.small:
            coef, rgb, err = singles[c.name]
            assert err == [0], c.name
        else:
            alone = jpeg.Decoded([c.data])
            coef, rgb = [a.cpu().numpy() for a in alone.coefficients(0)], alone.image(0).cpu().numpy()
        _assert_coefficients(d.coefficients(i), coef, c.name)
        _assert_coefficients(d.coefficients(i), c.coef, c.name)
        assert np.array_equal(d.image(i).cpu().numpy(), rgb), c.name
        if c.pixels:
            assert np.array_equal(rgb, c.pil), c.name


def test_batch_with_one_damaged_file(jpeg, batch):
    """the file of test_gpu_jpeg.py whose header claims more rows than its stream holds, among the others: it alone reports an
    error, every other image is what the clean batch gave"""
    cases, clean = batch
    good = jpeg_ref.encode(jpeg_ref.content(4, 47, 33), "420", 75)
    i = good.index(b"\xff\xc0")
    assert struct.unpack_from(">HH", good, i + 5) == (47, 33)
    bad = good[:i + 5] + struct.pack(">H", 95) + good[i + 7:]
    at = 70
    items = [c.data for c in cases]
    d = jpeg.Decoded(items[:at] + [bad] + items[at:])
    err = d.errors.cpu().tolist()
    assert err[at] != 0 and err[:at] + err[at + 1:] == [0] * len(cases)
    with pytest.raises(jpeg.CorruptJpeg):
        d.check()
    for k, c in enumerate(cases):
        j = k if k < at else k + 1
        assert torch.equal(d.image(j), clean.image(k)), c.name
        for a, b in zip(d.coefficients(j), clean.coefficients(k)):
            assert torch.equal(a, b), c.name
