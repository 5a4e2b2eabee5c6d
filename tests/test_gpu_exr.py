"""GPU tests of the OpenEXR reader: read_exr against the values the tests' writer (exr_ref.py) stored, bit for bit; the
predictor kernel against its numpy restatement; the training arena and the patch sampler on OpenEXR files against
dataset_ref.py; a Radiance file and an OpenEXR file of the same values give the same arena; one reader batch."""
import importlib

import numpy as np
import pytest
import torch

import dataset_ref as R
import exr_ref as X
from oracle import imageio as O
from test_dataset import write_dorf
from test_exr import KNOWN_RGB, known_file
from test_gpu_dataset import SHAPES, _check

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
E = pkg.exr
D = pkg.dataset
IO = pkg.hdr_io
K = pkg._ops


def _host(t):
    return t.detach().cpu().numpy()


def _stored(img, t):
    return X.half_values(img) if t == X.HALF else np.asarray(img, dtype=np.float32)


def _assert_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ" % what
    gb, wb = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = gb != wb
    assert not bad.any(), "%s: %d values differ, first %r vs %r" % (what, bad.sum(), got[~gn][bad][:4], want[~wn][bad][:4])


def _image(rng, h, w):
    img = np.exp(rng.normal(0.0, 2.0, (h, w))).astype(np.float32) * np.where(rng.random((h, w)) < 0.1, -1, 1).astype(np.float32)
    img[:, : 2 * w // 3] = 0.75                                 # flat two thirds: RLE / ZIP chunks compress
    img[h // 2] = rng.normal(0.0, 1e3, w)                       # a noisy row
    return img


def test_known_file(tmp_path):
    path, _, _ = known_file(tmp_path)
    _assert_bits(_host(E.read_exr(path)), KNOWN_RGB, "known")


WIDTHS = (1, 7, 513, 4100)
TYPES = {"half": (X.HALF, X.HALF, X.HALF), "float": (X.FLOAT, X.FLOAT, X.FLOAT), "mixed": (X.HALF, X.FLOAT, X.HALF)}
CASES = [(comp, order, tname) for comp in (X.NONE, X.RLE, X.ZIPS, X.ZIP) for order in (X.INC, X.DEC) for tname in TYPES]


@pytest.mark.parametrize("i", range(len(CASES)), ids=["c%d-o%d-%s" % c for c in CASES])
def test_read_exr_bit_exact(tmp_path, i):
    comp, order, tname = CASES[i]
    w = WIDTHS[i % len(WIDTHS)]                                 # every compression meets every width
    h = 19 if w > 1000 else 37                                  # not multiples of 16: the last ZIP chunk is short
    rng = np.random.default_rng(i)
    ch = {c: (_image(rng, h, w), t) for c, t in zip("RGB", TYPES[tname])}
    ch["A"] = (np.where(rng.random((h, w)) < 0.05, 0.5, 1.0).astype(np.float32), X.HALF)   # extra channels on both
    ch["Z"] = (np.floor(rng.random((h, w)) * 1.2).astype(np.float32) * 100, X.FLOAT)       # sides of B, G, R
    path = str(tmp_path / "x.exr")
    info = X.write_exr(path, ch, comp, order, origin=(-3, -11))
    if comp != X.NONE and w > 1:                                # a 1-pixel scanline never shrinks
        assert any(info["coded"])
    want = np.stack([_stored(*ch[c]) for c in "RGB"], axis=-1)
    _assert_bits(_host(E.read_exr(path)), want, "case %s, width %d" % (CASES[i], w))


def test_read_exr_raw_zip_chunks(tmp_path):
    rng = np.random.default_rng(3)
    h, w = 40, 300
    ch = {c: (rng.normal(0.0, 1e4, (h, w)).astype(np.float32), X.FLOAT) for c in "RGB"}
    path = str(tmp_path / "noise.exr")
    info = X.write_exr(path, ch, X.ZIP)
    assert not any(info["coded"])                               # incompressible: every chunk stored raw
    ch["G"][0][:16] = 2.0                                       # first chunk compresses, the others stay raw
    info = X.write_exr(path, ch, X.ZIP)
    assert info["coded"] == [True, False, False]
    _assert_bits(_host(E.read_exr(path)), np.stack([ch[c][0] for c in "RGB"], -1), "raw chunks")


def test_read_exr_special_values(tmp_path):
    half_bits = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x0400, 0x7bff, 0xfbff, 0x7c00, 0xfc00, 0x7e00, 0x7c01,
                          0xfe00, 0x3c00, 0x3555, 0x0200], dtype=np.uint16)
    halves = half_bits.view(np.float16).astype(np.float32)      # +-0, subnormals, 65504, +-inf, quiet / signalling NaN
    floats = np.array([0.0, -0.0, 1e-40, -1e-45, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan, 1.0, 1 / 3, 7e-39, 65504.0,
                       -2.5, 1e30, 5e-324], dtype=np.float32)
    h, w = 3, 16
    r = np.tile(halves, (h, 1))
    g = np.tile(floats, (h, 1))
    b = np.tile(halves[::-1], (h, 1))
    for comp in (X.NONE, X.RLE, X.ZIPS, X.ZIP):
        path = str(tmp_path / ("s%d.exr" % comp))
        X.write_exr(path, {"R": (r, X.HALF), "G": (g, X.FLOAT), "B": (b, X.HALF)}, comp)
        got = _host(E.read_exr(path))
        want = np.stack([r, g, b], -1)
        _assert_bits(got, want, "special values, compression %d" % comp)
        assert got.view(np.uint32)[0, 11, 0] == 0x7f802000      # signalling NaN payload kept (numpy's conversion)


@pytest.mark.parametrize("n", [1, 2, 3, 4095, 4096, 4097, 8191, 8192, 8193, 40000, 400001])
def test_unpredict_kernel_matches_restatement(n):
    """n = 8192, 8193: h = 4096 and 4097 pairs, a whole number of 256 x 8-pair steps and one pair more (both halves carry into a
    second step).  An EMPTY coded chunk lies between two others: its workgroup writes nothing and its neighbours keep their bytes."""
    rng = np.random.default_rng(n)
    chunks = [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), b"", bytes(range(256)) * 3, b"",
              rng.integers(0, 256, 7, dtype=np.uint8).tobytes()]
    coded = np.array([1, 1, 0, 0, 1], dtype=np.uint8)
    data = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
    dev = torch.device("cuda")
    got = _host(K.exr_unpredict(torch.from_numpy(data).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(coded).to(dev)))
    want = X.unpredict(chunks[0]) + X.unpredict(chunks[1]) + chunks[2] + chunks[3] + X.unpredict(chunks[4])
    assert offsets[1] == offsets[2] and offsets[3] == offsets[4] and len(want) == n + 768 + 7
    assert got.tobytes() == want


# --- the training arena ------------------------------------------------------------------------------------------
def _arena_rgb(rng, h, w):
    rgb = np.exp(rng.normal(0.0, 2.5, (h, w, 3))).astype(np.float32) * (1.0 + np.arange(3, dtype=np.float32))
    rgb[h // 3:h // 3 + 40, w // 4:w // 4 + 60] = 0.0
    rgb[:7, :5] *= 1e4
    rgb[h // 2:h // 2 + 30, :50] *= -1.0                        # negatives: the load clips them to 0
    return np.clip(rgb, -6e4, 6e4)                              # finite as HALF too


@pytest.fixture(scope="module")
def mixed_dir(tmp_path_factory):
    """the shapes of test_gpu_dataset.py: downscale (landscape), portrait, upscale and identity as OpenEXR, the two others
    Radiance"""
    d = tmp_path_factory.mktemp("mixed")
    rng = np.random.default_rng(30)
    expected = {}
    exr_kinds = {"big.hdr": (X.ZIP, (X.HALF,) * 3, X.DEC), "port.hdr": (X.ZIPS, (X.FLOAT,) * 3, X.INC),
                 "small.hdr": (X.RLE, (X.HALF, X.FLOAT, X.HALF), X.DEC), "square.hdr": (X.NONE, (X.FLOAT, X.HALF, X.HALF), X.INC)}
    for name, (h, w) in sorted(SHAPES.items()):
        rgb = _arena_rgb(rng, h, w)
        if name in exr_kinds:
            comp, types, order = exr_kinds[name]
            name = name.replace(".hdr", ".exr")
            ch = {c: (rgb[..., k], t) for k, (c, t) in enumerate(zip("RGB", types))}
            ch["A"] = (np.ones((h, w), np.float32), X.HALF)
            X.write_exr(str(d / name), ch, comp, order, origin=(5, -2))
            expected[name] = np.stack([_stored(*ch[c]) for c in "RGB"], -1)
        else:
            IO.write_hdr(str(d / name), O.rgbe_encode(np.abs(rgb)))
            expected[name] = IO.read_hdr(str(d / name))
    names = sorted(expected)
    return str(d), names, expected


def test_arena_matches_restatement(mixed_dir):
    d, names, expected = mixed_dir
    assert sum(n.endswith(".exr") for n in names) == 4
    ds = D.PatchHDRDataset(d, names, True)
    for f, name in enumerate(names):
        want, tap = R.load(expected[name])
        got = _host(ds.image(f))
        assert got.shape == want.shape and min(got.shape[:2]) == 512, name
        _check(got, want, tap, name)
        if name.endswith(".exr"):
            assert (got >= 0).all(), name
    assert ds.load_seconds["host_decode"] > 0 and ds.load_seconds["device"] > 0
    means = _host(ds.means)
    for f in range(len(names)):
        img = _host(ds.image(f))
        for p in (0, 1):
            ref = np.mean(R.window(img, p), dtype=np.float64)
            assert abs(means[2 * f + p] - ref) <= 1e-6 * ref, (f, p)
    rows = np.array([[idx, S, y0, x0, k, idx % 2, (idx // 2) % 2] for idx in range(len(ds)) if names[idx // 2].endswith(".exr")
                     for S, y0, x0, k in ((256, 0, 0, 0), (700, 443, 100, 1), (1024, 767, 767, 3))], dtype=np.int32)
    got = _host(ds.render(rows))
    for n, (idx, S, y0, x0, k, f0, f1) in enumerate(rows.tolist()):
        want, tap = R.patch(_host(ds.image(idx // 2)), idx, S, y0, x0, k, f0, f1, means[idx])
        _check(got[n], want, tap, str(rows[n].tolist()))


def test_radiance_and_openexr_give_the_same_arena(tmp_path):
    rng = np.random.default_rng(31)
    names = []
    for name, (h, w) in (("up", (300, 400)), ("same", (512, 700)), ("down", (1100, 900))):
        IO.write_hdr(str(tmp_path / (name + ".hdr")), O.rgbe_encode(np.abs(_arena_rgb(rng, h, w))))
        rgb = IO.read_hdr(str(tmp_path / (name + ".hdr")))
        X.write_exr(str(tmp_path / (name + ".exr")), {c: (rgb[..., k], X.FLOAT) for k, c in enumerate("RGB")}, X.ZIP)
        names += [name + ".hdr", name + ".exr"]
    ds = D.PatchHDRDataset(str(tmp_path), names, True)
    for f in range(0, len(names), 2):
        assert torch.equal(ds.image(f), ds.image(f + 1)), names[f]
        assert torch.equal(ds.means[2 * f:2 * f + 2], ds.means[2 * f + 2:2 * f + 4]), names[f]


def test_reader_batch_from_openexr_files(tmp_path):
    rng = np.random.default_rng(32)
    d = tmp_path / "exr"
    d.mkdir()
    for i, (h, w) in enumerate(((600, 900), (520, 700), (800, 512))):
        rgb = _arena_rgb(rng, h, w)
        X.write_exr(str(d / ("f%d.exr" % i)), {c: (rgb[..., k], X.HALF) for k, c in enumerate("RGB")}, (X.ZIP, X.NONE, X.ZIPS)[i])
    crf_path = str(tmp_path / "dorfCurves.txt")
    write_dorf(crf_path, n=201)
    hdr, crf, invcrf, t = D.RandDatasetReader(D.get_train_dataset(str(d), crf_path=crf_path), 4).read_batch_data()
    assert tuple(hdr.shape) == (4, 256, 256, 3) and tuple(crf.shape) == (4, 1024) and tuple(invcrf.shape) == (4, 1024)
    assert tuple(t.shape) == (4,)
    for x in (hdr, crf, invcrf, t):
        assert x.is_cuda and torch.isfinite(x).all()
