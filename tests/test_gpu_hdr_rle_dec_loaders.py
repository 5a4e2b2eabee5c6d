"""The loaders with hdr_rle="device" (the Radiance scanlines of all files decoded in one hdr_io.rle_decode_device) against the same
loaders with the default "host": the resident data, the statistics and a rendered batch are the same bits."""
import importlib
import os

import numpy as np
import pytest
import torch

import exr_ref as X

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
D, IO, HR = pkg.dataset, pkg.hdr_io, pkg.hdr_real


def _rgbe(rng, h, w):
    """smooth mantissas with a band of noise, exponents near 128: coded lines with runs and literals"""
    yy, xx = np.mgrid[0:h, 0:w]
    rgbe = np.stack([(xx // 3 + yy) % 256, (yy // 2) % 256, (xx + 2 * yy) % 256, 126 + (xx // 16) % 4], axis=-1).astype(np.uint8)
    rgbe[h // 3:h // 3 + 4] = rng.integers(1, 256, rgbe[h // 3:h // 3 + 4].shape)
    rgbe[..., 3] = np.clip(rgbe[..., 3], 120, 136)
    return rgbe


@pytest.fixture(scope="module")
def training_dir(tmp_path_factory):
    """five Radiance files -- portrait, landscape, square, one with flat lines (W = 7), one more -- and an OpenEXR file beside them"""
    d = str(tmp_path_factory.mktemp("hdr_train"))
    rng = np.random.default_rng(61)
    names = []
    for i, (h, w) in enumerate(((70, 40), (36, 90), (48, 48), (30, 7), (65, 129))):
        names.append("r%d.hdr" % i)
        IO.write_hdr(os.path.join(d, names[-1]), _rgbe(rng, h, w))
    ch = {c: ((0.5 + np.add.outer(np.arange(40), np.arange(64)) / 64.0).astype(np.float32), X.HALF) for c in "RGB"}
    X.write_exr(os.path.join(d, "e.exr"), ch, X.ZIP)
    return d, names[:2] + ["e.exr"] + names[2:]


def test_patch_dataset_is_the_same_bits(training_dir):
    d, names = training_dir
    a = D.PatchHDRDataset(d, names, True, seed=3)
    b = D.PatchHDRDataset(d, names, True, seed=3, hdr_rle="device")
    assert a.shapes == b.shapes and torch.equal(a.arena.view(torch.int32), b.arena.view(torch.int32))
    assert torch.equal(a.means.view(torch.int32), b.means.view(torch.int32))
    assert set(b.load_seconds) == set(a.load_seconds) == {"host_decode", "device"}
    params = a.draw(np.arange(len(a)), np.random.default_rng(5))
    assert torch.equal(a.render(params).view(torch.int32), b.render(params).view(torch.int32))
    for i in range(len(names)):
        assert torch.equal(a.image(i), b.image(i))


def test_hdr_real_folder_is_the_same_bits(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(62)
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "HDR_gt"))
    os.makedirs(os.path.join(root, "LDR_in"))
    for i, (h, w) in enumerate(((33, 47), (40, 52), (32, 32))):
        IO.write_hdr(os.path.join(root, "HDR_gt", "s%d.hdr" % i), _rgbe(rng, h, w))
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "LDR_in", "s%d.jpg" % i), quality=92)
    a = HR.HdrRealFolder(root, size=16, stride=8, seed=2)
    b = HR.HdrRealFolder(root, size=16, stride=8, seed=2, hdr_rle="device")
    assert a.files == b.files and a.shapes == b.shapes
    assert torch.equal(a.hdr_arena.view(torch.int32), b.hdr_arena.view(torch.int32)) and torch.equal(a.ldr_arena, b.ldr_arena)
    assert a.patches == b.patches and a.candidates == b.candidates and np.array_equal(a.extreme_counts, b.extreme_counts)
    assert np.array_equal(a.means.view(np.uint32), b.means.view(np.uint32)) and np.array_equal(a.keep, b.keep)
    assert set(b.load_seconds) == {"host_decode", "device"}
    params = a.draw(8)
    for x, y in zip(a.render(params), b.render(params)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_unknown_option_values_raise(training_dir, tmp_path):
    d, names = training_dir
    for fn in (lambda: D.PatchHDRDataset(d, names, True, hdr_rle="gpu"), lambda: D.HDRDataset(d, names, True, hdr_rle=None),
               lambda: HR.HdrRealFolder(str(tmp_path), hdr_rle="cuda"), lambda: IO.read_rgbe(os.path.join(d, names[0]), decoder="both")):
        with pytest.raises(ValueError, match="must be 'host' or 'device'"):
            fn()
    items = [D.HDRDataset(d, names, True, hdr_rle="device")[i] for i in range(len(names))]
    assert [type(it).__name__ for it in items] == ["Scanlines", "Scanlines", "Payload", "Scanlines", "Scanlines", "Scanlines"]
