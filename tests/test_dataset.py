"""CPU tests of the training-set reader (dataset.py of the reference): the RLE decoder, the DoRF tables, the parameter draws,
and the import without any data file present.  The pixel path runs on the device: tests/test_gpu_dataset.py."""
import ctypes
import importlib
import mmap
import os
import subprocess
import sys

import numpy as np
import pytest

import dataset_ref as R
from conftest import ROOT

pkg = importlib.import_module("singlehdr-tf2_amd")
D = pkg.dataset
IO = pkg.hdr_io
PKG_DIR = os.path.join(ROOT, "singlehdr-tf2_amd")


def _guarded(data):
    """`data` placed flush against a PROT_NONE page: a read past its end faults instead of passing silently"""
    page = mmap.PAGESIZE
    n = -(-max(len(data), 1) // page) * page
    mm = mmap.mmap(-1, n + page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base + n, page, 0) == 0
    start = base + n - len(data)
    ctypes.memmove(start, bytes(data), len(data))
    return mm, start


def _decode_guarded(data, h, w):
    mm, start = _guarded(data)
    out = np.empty((h, w, 4), dtype=np.uint8)
    lib = pkg._lib.load()
    n = lib.shdr_rgbe_rle_decode(ctypes.c_void_p(start), len(data), w, h, ctypes.c_void_p(out.ctypes.data))
    return n, out, mm


def _image(rng, h, w):
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    img[:, : w // 3] = img[:, :1]
    if h > 1:
        img[1, :, 3] = 128
    return img


@pytest.mark.parametrize("w", [1, 3, 7, 8, 9, 127, 128, 129, 130, 255, 256, 300, 1000])
def test_rle_decode_inverts_encode(w):
    rng = np.random.default_rng(w)
    img = _image(rng, 5, w)
    enc = IO.rle_encode(img)
    n, out, _ = _decode_guarded(enc, 5, w)
    assert n == len(enc)
    assert np.array_equal(out, img)
    assert np.array_equal(IO.rle_decode(enc, 5, w), img)


@pytest.mark.parametrize("run", [127, 128, 129, 255, 256, 257])
def test_rle_decode_long_runs_and_literals(run):
    w = 300
    img = np.zeros((2, w, 4), dtype=np.uint8)
    img[0, :run, 0] = 9                                         # a run longer than one code can hold
    img[0, :, 1] = np.arange(w) % 251                           # literal stretches of 128
    img[1] = np.random.default_rng(run).integers(0, 256, (w, 4))
    enc = IO.rle_encode(img)
    assert np.array_equal(_decode_guarded(enc, 2, w)[1], img)
    # hand-written: literal of 128, run of 127 + run of 45 for component 0; runs for 1-3
    line = bytes([2, 2, 1, 44]) + bytes([128]) + bytes(range(128)) + bytes([255, 7, 128 + 45, 8])
    line += bytes([128 + 127, 1, 128 + 127, 1, 128 + 46, 1]) * 3
    n, out, _ = _decode_guarded(line, 1, 300)
    assert n == len(line)
    assert out[0, :128, 0].tolist() == list(range(128)) and (out[0, 128:255, 0] == 7).all() and (out[0, 255:, 0] == 8).all()
    assert (out[0, :, 1:] == 1).all()


def test_rle_decode_rejects_truncated_and_corrupt():
    rng = np.random.default_rng(3)
    for h, w in ((3, 5), (3, 40), (2, 300)):
        img = _image(rng, h, w)
        enc = IO.rle_encode(img)
        for cut in sorted(set(np.linspace(0, len(enc) - 1, 25).astype(int).tolist())):
            n, _, _ = _decode_guarded(enc[:cut], h, w)
            assert n == -1, (h, w, cut)
            assert b"truncated" in pkg._lib.load().shdr_last_error()
            with pytest.raises(ValueError):
                IO.rle_decode(enc[:cut], h, w)
    head = bytes([2, 2, 0, 8])
    for bad in (head + bytes([128 + 9, 1]),                        # run past the end of the scanline
                head + bytes([9]) + bytes(9),                      # literal past the end
                head + bytes([128 + 5, 1, 4, 1, 2, 3, 4])):        # 5 + 4 > 8
        n, _, _ = _decode_guarded(bad + bytes(64), 1, 8)
        assert n == -1 and b"corrupt" in pkg._lib.load().shdr_last_error()


def test_read_hdr_unchanged_and_exr_refused(tmp_path):
    rng = np.random.default_rng(4)
    img = _image(rng, 6, 50)
    path = str(tmp_path / "a.hdr")
    IO.write_hdr(path, img)
    assert np.array_equal(IO.read_rgbe(path), img)
    assert np.array_equal(IO.read_hdr(path), IO.rgbe_decode(img))
    data = open(path, "rb").read()
    open(str(tmp_path / "t.hdr"), "wb").write(data[:-20])
    with pytest.raises(ValueError, match="t.hdr"):
        IO.read_hdr(str(tmp_path / "t.hdr"))
    open(str(tmp_path / "x.exr"), "wb").write(b"\x76\x2f\x31\x01" + bytes(100))
    with pytest.raises(ValueError, match="OpenEXR"):
        IO.read_rgbe(str(tmp_path / "x.exr"))


def write_dorf(path, n=201, seed=0, strict=True):
    """a DoRF-layout file: per curve a name, a type, 'I =', irradiance, 'B =', brightness"""
    rng = np.random.default_rng(seed)
    curves = []
    with open(path, "w") as f:
        for i in range(n):
            b = np.cumsum(rng.random(1024) + (0.01 if strict else 0.0)) if strict else np.sort(np.round(rng.random(1024), 2))
            b = ((b - b[0]) / (b[-1] - b[0])).astype(np.float32)
            curves.append(b)
            f.write("curve-%d\ngraph\nI =\n%s\nB =\n%s\n" % (
                i, " ".join("%.6e" % v for v in np.linspace(0, 1, 1024)), " ".join("%.9e" % v for v in b)))
    return np.float32([[float("%.9e" % v) for v in c] for c in curves])


def test_dorf_split_and_invcrf(tmp_path):
    from scipy.interpolate import interp1d
    path = str(tmp_path / "dorfCurves.txt")
    curves = write_dorf(path)
    test, train = D._get_crf_list(path)
    want = curves.copy()
    np.random.RandomState(730).shuffle(want)
    assert test.shape == (10, 1024) and train.shape == (191, 1024)
    assert np.array_equal(test, want[-10:]) and np.array_equal(train, want[:-10])
    assert test.dtype == np.float32
    inv = D._get_invcrf_list(train[:20])
    for c, got in zip(train[:20], inv):
        rf = c.copy()
        rf[0], rf[-1] = 0.0, 1.0
        ref = interp1d(rf, np.linspace(0.0, 1.0, 1024))(np.linspace(0.0, 1.0, 1024))
        assert np.abs(got - ref).max() <= 1e-6
    crf, invcrf, t = D.crf_tables("train", path)
    assert np.array_equal(crf, train) and t.shape == (600,) and t.dtype == np.float32
    assert t[0] == np.float32(0.125) and t[-1] == np.float32(8.0)
    vcrf, vinv, vt = D.crf_tables("vali", path)
    assert vcrf.shape == (10, 1024) and vt.shape == (5,) and len(D.crf_tables("test", path)[2]) == 7
    assert np.array_equal(vinv, np.array(D._get_invcrf_list(vcrf)))           # the two shuffles keep the pairs together


def test_dorf_lookup_and_missing_file(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    if not os.path.exists(os.path.join(PKG_DIR, "dorfCurves.txt")):
        with pytest.raises(FileNotFoundError, match="dorfCurves.txt"):
            D.crf_tables("train")
    write_dorf(str(tmp_path / "dorfCurves.txt"), n=20)
    assert D.crf_tables("train")[0].shape == (10, 1024)             # found in the current directory


def test_param_draws_cover_their_ranges():
    s = D.ParamSampler(2 * 7, 191, 600, True, seed=5, rank=0)
    p = np.concatenate([s.draw(32) for _ in range(200)])
    idx, S, y0, x0, k, f0, f1, ci, ti = p.T
    assert set(k.tolist()) == {0, 1, 2, 3} and set(f0.tolist()) == {0, 1} and set(f1.tolist()) == {0, 1}
    assert S.min() == 256 and S.max() == 1024
    assert ((S == 256) <= ((y0 == 0) & (x0 == 0))).all()
    big = S > 256
    assert (x0[big] < S[big] - 256).all() and (y0[big] < S[big] - 256).all() and x0.min() == 0
    assert (y0 >= 0).all() and (x0 + 256 <= S).all()
    assert ci.min() == 0 and ci.max() == 190 and ti.min() == 0 and ti.max() == 599
    # every epoch is a permutation of the 14 patches
    for e in range(len(idx) // 14):
        assert sorted(idx[14 * e:14 * e + 14].tolist()) == list(range(14))
    v = D.ParamSampler(20, 10, 5, False).draw(40)
    assert (v[:, D.P_S] == 512).all() and not v[:, [D.P_Y0, D.P_X0, D.P_K, D.P_FLIP0, D.P_FLIP1]].any()


def test_param_draws_seeded_per_rank(tmp_path):
    a = D.ParamSampler(100, 191, 600, True, seed=3, rank=0)
    b = D.ParamSampler(100, 191, 600, True, seed=3, rank=0)
    c = D.ParamSampler(100, 191, 600, True, seed=3, rank=1)
    pa, pb, pc = a.draw(64), b.draw(64), c.draw(64)
    assert np.array_equal(pa, pb) and not np.array_equal(pa, pc)
    # training draws index the training curves only: none of them is a test curve
    path = str(tmp_path / "dorfCurves.txt")
    write_dorf(path, n=201, seed=1)
    crf, _, _ = D.crf_tables("train", path)
    test, _, _ = D.crf_tables("test", path)
    rows = crf[np.concatenate([a.draw(64)[:, D.P_CRF] for _ in range(20)])]
    assert not (rows[:, None, :] == test[None, :, :]).all(-1).any()


def test_restatement_resize_rule():
    x = np.random.default_rng(0).random((7, 9, 3)).astype(np.float32)
    same, tap = R.resize_linear(x, (7, 9))
    assert np.array_equal(same, x) and (tap >= x).all()            # copies; the bar counts the zero-weight taps too
    y, _ = R.resize_linear(x, (14, 18))                              # upscale: border rows / columns are copies
    assert np.allclose(y[0, 0], x[0, 0], rtol=1e-6) and np.allclose(y[-1, -1], x[-1, -1], rtol=1e-6)
    half, _ = R.resize_linear(np.arange(8, dtype=np.float32).reshape(1, 8, 1).repeat(2, 0), (1, 4))
    assert half[0, :, 0].tolist() == [0.5, 2.5, 4.5, 6.5]          # scale 2: weights (0.5, 0.5)
    assert D.resized_shape(600, 900) == (512, 768) and D.resized_shape(1500, 1500) == (512, 512)
    assert D.resized_shape(300, 200) == (768, 512)


def test_restatement_edge_axes():
    """the clamp rules on 1- and 2-pixel axes: a one-pixel axis has both taps on its only line; the horizontal rule gives the edge
    tap the whole weight, the vertical rule keeps the weight and clamps the rows"""
    for clamp in (False, True):
        s0, s1, f = R._axis(5, 1, clamp)
        assert s0.tolist() == [0] * 5 == s1.tolist()
        assert (f == 0).all() if clamp else (f != 0).any()
    s0, s1, f = R._axis(7, 2, True)
    assert s0.tolist() == [0, 0, 0, 0, 0, 1, 1] and s1.tolist() == [1] * 7
    assert (f[[0, 1, 5, 6]] == 0).all() and f[3] == 0.5 and 0 < f[2] < f[3] < f[4] < 1
    s0, s1, g = R._axis(7, 2, False)
    assert s0.tolist() == [0, 0, 0, 0, 0, 1, 1] and s1.tolist() == [0, 0, 1, 1, 1, 1, 1]
    assert (g[[0, 1, 5, 6]] != 0).all() and np.array_equal(g[2:5], f[2:5])
    x = np.float32([[[1.0, 2.0, 3.0]]])
    y, _ = R.resize_linear(x, (4, 5))
    assert np.abs(y - x).max() <= 2.0 ** -22                    # v (1 - f) + v f: the value up to the two roundings
    y, _ = R.resize_linear(np.float32([[[0.0], [1.0]], [[2.0], [3.0]]]), (7, 7))
    assert y[0, 0, 0] == 0.0 and abs(y[-1, -1, 0] - 3.0) <= 2.0 ** -21 and (np.diff(y[..., 0], axis=1) >= 0).all()


def test_restatement_decoders():
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, size=(9, 11, 4), dtype=np.uint8)
    img[0, :5, 3] = [0, 1, 9, 128, 255]
    img[1, :2, :3] = [[0, 0, 0], [255, 255, 255]]
    img[1, :2, 3] = 1
    bgr = R.rgbe_bgr(img)
    assert bgr.dtype == np.float32 and np.array_equal(bgr, IO.rgbe_decode(img)[:, :, ::-1])
    assert (bgr[0, 0] == 0).all() and bgr[1, 1, 0] == np.float32(255 * 2.0 ** -135) and 0 < bgr[1, 1, 0] < np.finfo(np.float32).tiny
    assert np.isfinite(bgr).all() and bgr[0, 4].max() <= 255 * 2.0 ** 119
    h = np.arange(65536, dtype=np.uint16)
    f = R.half_bits_to_float(h)
    ref = h.view(np.float16).astype(np.float32)
    finite = ~np.isnan(ref)
    assert np.array_equal(f[finite].view(np.uint32), ref[finite].view(np.uint32))          # +-0, subnormals, +-inf included
    assert np.isnan(f[~finite]).all() and f.view(np.uint32)[0x7C01] == 0x7F802000 and f.view(np.uint32)[0xFE00] == 0xFFC00000
    c = R.clip0(np.float32([-1.0, -0.0, 0.5, np.inf, -np.inf, np.nan]))
    assert c.view(np.uint32)[:5].tolist() == [0, 0x80000000, 0x3F000000, 0x7F800000, 0] and np.isnan(c[5])


def test_cropped_patch_equals_full_patch():
    """dataset_ref.patch_crop (the reference of tests/test_gpu_dataset_exact.py, which evaluates only the crop's rows and columns)
    against patch() at P = 256 on the parameter table of the sampler's GPU test: the same bits"""
    from test_gpu_dataset import _forced_params
    rng = np.random.default_rng(40)
    imgs = [np.exp(rng.normal(0.0, 2.5, hw + (3,))).astype(np.float32) for hw in ((512, 530), (540, 512))]
    params = _forced_params(2)
    assert len(params) == 2 * 8 + 64 and {tuple(r) for r in params[:, 4:7].tolist()} == {(k, a, b) for k in range(4) for a in (0, 1)
                                                                                        for b in (0, 1)}
    for idx, S, y0, x0, k, f0, f1 in params.tolist():
        img, mean = imgs[(idx // 2) % 2], np.float32(0.37 + idx)
        full, tap = R.patch(img, idx, S, y0, x0, k, f0, f1, mean)
        crop, ctap = R.patch_crop(img, idx, S, y0, x0, k, f0, f1, mean, 256)
        assert np.array_equal(full.view(np.uint32), crop.view(np.uint32)), (idx, S, y0, x0, k, f0, f1)
        assert np.array_equal(tap, ctap)


def test_import_without_data_files(tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dataset import get_train_dataset, RandDatasetReader\n"
            "import dataset; print(dataset.RandDatasetReader.__name__)\n" % PKG_DIR)
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, "-c", code], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "RandDatasetReader" in r.stdout
    assert "dataset" in pkg.__all__
