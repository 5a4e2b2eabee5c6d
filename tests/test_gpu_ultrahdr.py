"""GPU tests of gain-map JPEG files (ultrahdr.py) on the device routes, and of output_format="ultrahdr" in the file loop (hdr_io): the
device routes against the host routes byte for byte, the files of the loop against Pillow, xml.etree and the round-trip bound of
test_ultrahdr_container.py.  No foreign Ultra HDR reader has opened these files."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import gainmap_ref as R
from oracle import nets

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _mixed():
    by_content = {name: R.cases(name) for name in R.CONTENTS}
    picks = [by_content[R.CONTENTS[i % len(R.CONTENTS)]][i] for i in range(0, len(R.SHAPES) * len(R.FACTORS), 3)]
    sdrs = [c["sdr"] for c in picks]
    hdrs = [c["hdr"][..., ::-1].copy() if c["reverse"] else c["hdr"] for c in picks]
    return sdrs, hdrs, [c["factor"] for c in picks]


def test_device_route_writes_the_host_route_s_bytes(shdr):
    U = shdr.ultrahdr
    sdr, hdr = R.content("ramp", (65, 130), 1)
    one = U.encode([dev(hdr)], [dev(sdr)])
    assert one == U.encode([hdr], [sdr], encoder="host")
    swapped = np.ascontiguousarray(hdr[..., ::-1])
    assert U.encode([dev(swapped)], [dev(sdr)], factor=2, hdr_scale=0.5, reverse_channels=True, map_quality=95) == \
        U.encode([hdr], [sdr], factor=2, hdr_scale=0.5, map_quality=95, encoder="host")
    sdrs, hdrs, factors = _mixed()
    opts = dict(factor=factors, base_options=dict(quality=90, subsampling="422"))
    got = U.encode([dev(h) for h in hdrs], [dev(s) for s in sdrs], **opts)
    assert got == U.encode(hdrs, sdrs, encoder="host", **opts)
    for data, s, f in zip(got, sdrs, factors):
        with Image.open(io.BytesIO(data)) as im:
            assert im.format == "MPO" and im.n_frames == 2 and im.size == (s.shape[1], s.shape[0])
            im.seek(1)
            assert im.size == (-(-s.shape[1] // f), -(-s.shape[0] // f))


def test_device_decoder_is_the_pil_route_bit_for_bit(shdr):
    U = shdr.ultrahdr
    sdrs, hdrs, factors = _mixed()
    files = U.encode(hdrs, sdrs, factor=factors, encoder="host")
    for boost in (None, 1.7):
        a = U.decode(files, display_boost=boost, decoder="device")
        b = U.decode(files, display_boost=boost, decoder="pil")
        c = U.decode(files, display_boost=boost, decoder="host")
        for x, y, z, s in zip(a, b, c, sdrs):
            assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == s.shape
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            assert np.array_equal(x.cpu().numpy().view(np.uint32), z.view(np.uint32))


@pytest.fixture(scope="module")
def loop(shdr, tmp_path_factory):
    """a reconstructor with seeded nets as test_gpu_io.py builds them, and a folder with one 40 x 56 JPEG and one PNG of it"""
    P = {k: nets.init_params(getattr(nets, k + "_spec")(), 40 + i) for i, k in enumerate(("deq", "lin", "hal", "ref"))}
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    ms = {k: getattr(shdr, mods[k]).model().load_numpy(P[k]) for k in mods}
    recon = shdr.hdr_io.HdrReconstructor(shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"]))
    rng = np.random.default_rng(5)
    img = np.clip(rng.random((4, 7, 3)).repeat(10, axis=0).repeat(8, axis=1) + rng.normal(size=(40, 56, 3)) * 0.03, 0, 1)
    src = tmp_path_factory.mktemp("ultrahdr_in")
    Image.fromarray((img * 255).astype(np.uint8)).save(str(src / "scene.jpg"), quality=93)
    Image.fromarray((img * 255).astype(np.uint8)).save(str(src / "flat.png"))
    return recon, src


def _check_loop_file(shdr, recon, path, src_path, factor):
    """a file of the loop: named .jpg, a two-frame MPO, the input's scan verbatim (JPEG input), the map of the expected size"""
    U = shdr.ultrahdr
    assert path.endswith(".jpg")
    with open(path, "rb") as f:
        data = f.read()
    sdr = shdr.hdr_io.read_ldr(src_path)
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == "MPO" and im.n_frames == 2 and im.size == (56, 40)
        if src_path.endswith(".jpg"):
            assert np.array_equal(np.array(im.convert("RGB")), sdr)
        im.seek(1)
        assert im.size == (-(-56 // factor), -(-40 // factor))
    if src_path.endswith(".jpg"):
        with open(src_path, "rb") as f:
            scan = f.read()
        scan = scan[scan.index(b"\xff\xda"):-2]
        assert data.count(scan) == 1
    return data


def _check_round_trip(shdr, recon, data, src_path):
    """at factor 1 and map quality 100: the decoded file against s * the estimate of reconstruct_device, within the round-trip bound"""
    K, U = shdr._ops, shdr.ultrahdr
    primary = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
    y = recon.reconstruct_device(shdr.hdr_io.read_ldr(src_path)).contiguous()
    images, _, _ = K.gainmap_images([(40, 56)], 1)
    codes, meta = K.gainmap_encode(dev(primary).reshape(-1), y.reshape(-1), images, reverse_channels=True)
    meta = meta.cpu().numpy().view(K.GAINMAP_META_DTYPE)[0]
    decoded = np.array(Image.open(io.BytesIO(U.split(data)[1])).convert("RGB")).astype(np.float64)
    J = np.abs(decoded - codes.cpu().numpy().reshape(40, 56, 3))
    T, bound = R.round_trip_bound(primary, y.cpu().numpy()[..., ::-1], float(meta["scale"]), float(meta["gain_min"]), float(meta["gain_max"]), J)
    got = U.decode([data], decoder="device")[0].cpu().numpy()
    err = np.abs(got.astype(np.float64) - T)
    assert (err <= bound).all(), float((err / bound).max())
    fields = U.split(data)[2]
    assert fields["GainMapMin"] == float(meta["gain_min"]) and fields["GainMapMax"] == float(meta["gain_max"])


def test_file_loop_writes_gain_map_files(shdr, loop, tmp_path):
    recon, src = loop
    jpg, png = str(src / "scene.jpg"), str(src / "flat.png")
    exact = dict(factor=1, map_quality=100)
    one = str(tmp_path / "one.jpg")
    recon.reconstruct_file(jpg, one, output_format="ultrahdr", ultrahdr_options=exact)
    _check_round_trip(shdr, recon, _check_loop_file(shdr, recon, one, jpg, 1), jpg)
    dflt = str(tmp_path / "default.jpg")
    recon.reconstruct_file(jpg, dflt, output_format="ultrahdr", decoder="device", preview_path=str(tmp_path / "p.png"))
    _check_loop_file(shdr, recon, dflt, jpg, 4)
    assert os.path.getsize(str(tmp_path / "p.png")) > 0
    outs = [str(tmp_path / "a.jpg"), str(tmp_path / "b.jpg")]
    recon.reconstruct_files([jpg, png], outs, output_format="ultrahdr", ultrahdr_options=exact)
    with open(outs[0], "rb") as f, open(one, "rb") as g:
        assert f.read() == g.read()                                  # the batch writes what the single call writes
    _check_round_trip(shdr, recon, _check_loop_file(shdr, recon, outs[1], png, 1), png)       # a PNG input: the base is coded
    written = recon.reconstruct_dir(str(src), str(tmp_path / "out"), pattern="*.*", verbose=False, output_format="ultrahdr", group=2,
                                    ultrahdr_options=exact)
    assert [os.path.basename(p) for p in written] == ["flat.jpg", "scene.jpg"]
    with open(written[1], "rb") as f, open(one, "rb") as g:
        assert f.read() == g.read()
    _check_loop_file(shdr, recon, written[0], png, 1)
    with pytest.raises(ValueError, match="overwrite the inputs"):
        recon.reconstruct_dir(str(src), str(src / "." / ""), verbose=False, output_format="ultrahdr")
    with pytest.raises(ValueError, match="ultrahdr_options takes"):
        recon.reconstruct_file(jpg, one, output_format="ultrahdr", ultrahdr_options=dict(base=[b""]))
    with pytest.raises(ValueError, match="'hdr', 'exr' or 'ultrahdr'"):
        recon.reconstruct_file(jpg, one, output_format="tiff")


def test_the_other_formats_write_what_they_wrote(shdr, loop, tmp_path):
    """the calls with their defaults against the steps they were made of before output_format="ultrahdr" existed"""
    recon, src = loop
    IO, K = shdr.hdr_io, shdr._ops
    jpg = str(src / "scene.jpg")
    y = recon.reconstruct_device(IO.read_ldr(jpg))
    want_hdr, want_exr = str(tmp_path / "want.hdr"), str(tmp_path / "want.exr")
    IO.write_hdr(want_hdr, K.rgbe_encode(y, reverse_channels=True).cpu().numpy(), encoder="host")
    shdr.exr.write_exr(want_exr, y, encoder="host", reverse_channels=True)

    def same(a, b):
        with open(a, "rb") as f, open(b, "rb") as g:
            return f.read() == g.read()
    recon.reconstruct_file(jpg, str(tmp_path / "file.hdr"))
    assert same(str(tmp_path / "file.hdr"), want_hdr)
    recon.reconstruct_files([jpg], [str(tmp_path / "files.hdr")])
    assert same(str(tmp_path / "files.hdr"), want_hdr)
    recon.reconstruct_files([jpg], [str(tmp_path / "files_dev.hdr")], encoder="device")
    assert same(str(tmp_path / "files_dev.hdr"), want_hdr)
    recon.reconstruct_file(jpg, str(tmp_path / "file.exr"), output_format="exr")
    assert same(str(tmp_path / "file.exr"), want_exr)
    written = recon.reconstruct_dir(str(src), str(tmp_path / "dir"), verbose=False)
    assert [os.path.basename(p) for p in written] == ["scene.hdr"] and same(written[0], want_hdr)
    written = recon.reconstruct_dir(str(src), str(tmp_path / "dir_exr"), verbose=False, output_format="exr", encoder="device", group=4)
    assert [os.path.basename(p) for p in written] == ["scene.exr"]
    assert torch.equal(shdr.exr.read_exr(written[0]), shdr.exr.read_exr(want_exr))
