"""OpenEXR output with encoder="device_lz" (exr.encode_exr, csrc/deflate_lz.hip, hdr_io's output_format="exr"): the files read back to
the pixels of the encoder="host" files, and their chunks are the host routine's streams of the predicted bytes of tests/exr_ref.py."""
import importlib
import zlib

import numpy as np
import pytest

import exr_ref as R
from test_gpu_exr_write import COMPS, dev, file_chunks, noisy_ramp, ref_file, same_bits, stored_values, wild_image

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
EXR, IO, K = pkg.exr, pkg.hdr_io, pkg._ops


def smooth_ramp(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    return np.stack((1.0 + xx / w + yy / h, 0.5 + 0.25 * xx / w + 0.1 * yy / h, 2.0 + 3.0 * (xx + yy) / (h + w)), axis=-1).astype(np.float32)


def images():
    return [wild_image(1, 1, 1), wild_image(5, 17, 2), noisy_ramp(48, 64, 3), smooth_ramp(40, 64), noisy_ramp(33, 70, 4)]


def read(tmp_path, data):
    path = str(tmp_path / "got.exr")
    with open(path, "wb") as f:
        f.write(data)
    return EXR.read_exr(path).cpu().numpy()


@pytest.mark.parametrize("compression", ["zips", "zip"])
@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_files_read_back_and_hold_the_host_streams(tmp_path, pixel_type, compression):
    imgs = images()
    files = EXR.encode_exr([dev(a) for a in imgs], pixel_type, compression, "device_lz")
    host_files = EXR.encode_exr([dev(a) for a in imgs], pixel_type, compression, "host")
    any_coded = False
    for img, data, host in zip(imgs, files, host_files):
        got = read(tmp_path, data)
        assert same_bits(got, read(tmp_path, host)) and same_bits(got, stored_values(img, pixel_type))
        _, rep = ref_file(tmp_path / "ref.exr", img, pixel_type, compression)
        lines = R.LINES[COMPS[compression]]
        for c, ((y, stored), raw) in enumerate(zip(file_chunks(data, rep), rep["chunks"])):
            z = K.deflate_lz_host(R.predict(raw))
            assert y == c * lines and stored == (z if len(z) < len(raw) else raw), (img.shape, c)
            if len(z) < len(raw):
                assert zlib.decompress(stored) == R.predict(raw)
                any_coded = True
    assert any_coded


def test_smooth_zip_file_is_far_smaller_than_the_huffman_only_one():
    img = dev(smooth_ramp(64, 256))
    lz, huffman = (EXR.encode_exr(img, "half", "zip", e)[0] for e in ("device_lz", "device"))
    assert 2 * len(lz) < len(huffman)


@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_none_files_are_unchanged(tmp_path, pixel_type):
    imgs = [wild_image(17, 65, 1), wild_image(1, 1, 2)]
    files = EXR.encode_exr([dev(a) for a in imgs], pixel_type, "none", "device_lz")
    for img, data in zip(imgs, files):
        assert data == ref_file(tmp_path / "r.exr", img, pixel_type, "none")[0]
    assert files == EXR.encode_exr([dev(a) for a in imgs], pixel_type, "none", "host")


def test_write_exr_and_refusals(tmp_path):
    img = noisy_ramp(17, 65, 9)
    a, b = str(tmp_path / "a.exr"), str(tmp_path / "b.exr")
    EXR.write_exr(a, dev(img), encoder="device_lz")
    EXR.write_exr(b, dev(img))
    assert same_bits(EXR.read_exr(a).cpu().numpy(), EXR.read_exr(b).cpu().numpy())
    with pytest.raises(ValueError, match="'host', 'device' or 'device_lz'"):
        EXR.encode_exr(dev(img), encoder="lz")
    with pytest.raises(ValueError, match="'host', 'device' or 'device_lz'"):
        IO.HdrReconstructor(lambda x: x).reconstruct_file("a.jpg", "b.exr", encoder="lz", output_format="exr")


@pytest.fixture(scope="module")
def recon():
    from oracle import nets
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    ms = {k: getattr(pkg, mods[k]).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), 60 + i)) for i, k in enumerate(mods)}
    return IO.HdrReconstructor(pkg.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"]))


def test_file_loop_passes_the_encoder_through(recon, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(13)
    paths = []
    for i, (h, w) in enumerate(((64, 64), (40, 50))):
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack((xx * 255.0 / w, yy * 255.0 / h, np.full((h, w), 90.0)), axis=-1)
        paths.append(str(tmp_path / ("in%d.png" % i)))
        Image.fromarray(np.clip(base + rng.normal(0, 3, base.shape), 0, 255).astype(np.uint8)).save(paths[-1])
    lz = [str(tmp_path / ("lz%d.exr" % i)) for i in range(2)]
    host = [str(tmp_path / ("host%d.exr" % i)) for i in range(2)]
    recon.reconstruct_files(paths, lz, output_format="exr", encoder="device_lz")
    recon.reconstruct_files(paths, host, output_format="exr", encoder="host")
    for a, b, src in zip(lz, host, paths):
        assert same_bits(EXR.read_exr(a).cpu().numpy(), EXR.read_exr(b).cpu().numpy())
        want = recon.reconstruct_device(IO.read_ldr(src)).cpu().numpy()[..., ::-1]
        assert same_bits(EXR.read_exr(a).cpu().numpy(), stored_values(want, "half"))
    one = str(tmp_path / "one.exr")
    recon.reconstruct_file(paths[1], one, output_format="exr", encoder="device_lz")
    assert open(one, "rb").read() == open(lz[1], "rb").read()
    d = tmp_path / "dir"
    written = recon.reconstruct_dir(str(tmp_path), str(d), pattern="in*.png", verbose=False, encoder="device_lz", group=2, output_format="exr")
    assert [open(p, "rb").read() for p in written] == [open(p, "rb").read() for p in lz]
    for call in (lambda: recon.reconstruct_file(paths[0], str(tmp_path / "x.hdr"), encoder="device_lz"),
                 lambda: recon.reconstruct_files(paths, [str(tmp_path / "x.hdr")] * 2, encoder="device_lz", output_format="hdr"),
                 lambda: recon.reconstruct_dir(str(tmp_path), str(d), pattern="in*.png", encoder="device_lz"),
                 lambda: IO.write_hdr(str(tmp_path / "x.hdr"), np.zeros((2, 2, 4), np.uint8), encoder="device_lz")):
        with pytest.raises(ValueError, match="OpenEXR output"):
            call()
    assert not (tmp_path / "x.hdr").exists()
