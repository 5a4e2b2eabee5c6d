"""OpenEXR output (exr.encode_exr / write_exr, csrc/exr_write.hip, csrc/deflate.hip, hdr_io's output_format="exr") against the
independent numpy writer tests/exr_ref.py, zlib's inflate and the product's own reader: bytes and values exactly, never a tolerance."""
import importlib
import struct
import zlib

import numpy as np
import pytest
import torch

import exr_ref as R

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
EXR, IO, K = pkg.exr, pkg.hdr_io, pkg._ops

WIDTHS = (1, 2, 7, 64, 65, 301)
HEIGHTS = (1, 15, 16, 17, 33)
SPECIALS = np.array([0.0, -0.0, 6e-8, 65504.0, 65519.0, 65520.0, 1e30, np.inf, np.nan], dtype=np.float32)
PTYPES = {"half": R.HALF, "float": R.FLOAT}
COMPS = {"none": R.NONE, "zips": R.ZIPS, "zip": R.ZIP}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def wild_image(h, w, seed):
    """random normal data times exp of a ramp (values from 1e-4 to beyond the HALF range, both signs), the specials in front"""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(-9.0, 13.0, h * w * 3, dtype=np.float32).reshape(h, w, 3)
    img = (rng.standard_normal((h, w, 3)).astype(np.float32) * np.exp(ramp)).astype(np.float32)
    flat = img.reshape(-1)
    k = min(flat.size, 2 * SPECIALS.size)
    flat[:k] = np.concatenate([SPECIALS, -SPECIALS])[:k]
    return img


def noisy_ramp(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack((1.0 + xx / w + yy / h, 0.5 + 0.25 * xx / w + 0.1 * yy / h, 2.0 + 3.0 * (xx + yy) / (h + w)), axis=-1)
    return (base * (1.0 + 0.02 * rng.standard_normal(base.shape))).astype(np.float32)


def white_noise(h, w, seed):
    """random bits (inf and NaN patterns moved one exponent down, so every sample is finite): as FLOAT samples nothing shrinks them"""
    bits = np.random.default_rng(seed).integers(0, 2 ** 32, (h, w, 3), dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] ^= 0x00800000
    return bits.view(np.float32)


def stored_values(img, pixel_type, saturate=True):
    """what the file holds for float data img, as float32"""
    if pixel_type == "float":
        return img
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.where(np.isfinite(img), np.clip(img, -65504.0, 65504.0), img) if saturate else img
        return R.half_values(x)


def ref_file(path, img, pixel_type, compression, reverse=False, saturate=True, chunk_hook=None):
    """the independent writer on the same arrays: (file bytes, its report)"""
    x = img
    if pixel_type == "half" and saturate:
        with np.errstate(invalid="ignore"):
            x = np.where(np.isfinite(img), np.clip(img, -65504.0, 65504.0), img)
    names = "BGR" if reverse else "RGB"
    with np.errstate(over="ignore", invalid="ignore"):
        rep = R.write_exr(str(path), {names[i]: (x[..., i], PTYPES[pixel_type]) for i in range(3)}, compression=COMPS[compression],
                          chunk_hook=chunk_hook)
    with open(str(path), "rb") as f:
        return f.read(), rep


def file_chunks(data, rep):
    """(y, stored bytes) of every chunk of a file with the header length and chunk count of the reference's report"""
    n = len(rep["chunks"])
    table = struct.unpack_from("<%dQ" % n, data, rep["table_at"])
    out = []
    for c in range(n):
        y, size = struct.unpack_from("<ii", data, table[c])
        out.append((y, data[table[c] + 8:table[c] + 8 + size]))
    assert table[0] == rep["table_at"] + 8 * n and table[-1] + 8 + len(out[-1][1]) == len(data)
    return out


# ---- packer -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wild_images():
    return [wild_image(h, w, 100 * h + w) for h in HEIGHTS for w in WIDTHS]


@pytest.mark.parametrize("saturate", [True, False], ids=["saturate", "plain"])
@pytest.mark.parametrize("reverse", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("lines", [1, 16])
@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_pack_planar_and_predicted_bytes(wild_images, tmp_path, pixel_type, lines, reverse, saturate):
    """all 30 shapes in ONE launch; every chunk's scanline bytes and predicted bytes against exr_ref"""
    packed = K.exr_pack([dev(a) for a in wild_images], PTYPES[pixel_type], lines, reverse_channels=reverse, saturate=saturate)
    planar, predicted, off = packed.planar.cpu().numpy(), packed.predicted.cpu().numpy(), packed.chunk_off
    c = 0
    for i, img in enumerate(wild_images):
        _, rep = ref_file(tmp_path / "r.exr", img, pixel_type, "zip" if lines == 16 else "none", reverse, saturate)
        assert packed.table[0][i] == c
        for raw in rep["chunks"]:
            assert off[c + 1] - off[c] == len(raw), (img.shape, c)
            assert planar[off[c]:off[c + 1]].tobytes() == raw, (img.shape, c)
            assert predicted[off[c]:off[c + 1]].tobytes() == R.predict(raw), (img.shape, c)
            c += 1
    assert c == off.size - 1 and off[-1] == planar.size


def test_pack_accepts_a_batch_tensor_and_skips_the_predictor(wild_images):
    img = np.stack([wild_image(17, 7, s) for s in range(3)])
    a = K.exr_pack(dev(img), R.HALF, 16, predict=False)
    b = K.exr_pack([dev(x) for x in img], R.HALF, 16)
    assert a.predicted is None and torch.equal(a.planar, b.planar) and np.array_equal(a.chunk_off, b.chunk_off)
    assert a.table[0].tolist() == [0, 2, 4, 6] and a.table[1].tolist() == [0, 119, 238, 357]


# ---- files --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_none_files_equal_the_reference_writer(tmp_path, pixel_type):
    imgs = [wild_image(17, 65, 1), wild_image(1, 1, 2), wild_image(33, 7, 3)]
    for encoder in ("host", "device"):
        one = EXR.encode_exr(dev(imgs[0]), pixel_type, "none", encoder)
        three = EXR.encode_exr([dev(a) for a in imgs], pixel_type, "none", encoder)
        assert len(one) == 1 and len(three) == 3 and one[0] == three[0]
        for img, data in zip(imgs, three):
            assert data == ref_file(tmp_path / "r.exr", img, pixel_type, "none")[0]
    rev = EXR.encode_exr(dev(imgs[0]), pixel_type, "none", reverse_channels=True, saturate=False)[0]
    assert rev == ref_file(tmp_path / "r.exr", imgs[0], pixel_type, "none", reverse=True, saturate=False)[0]


def huffman_hook(rep_chunks):
    """exr_ref chunk hook that stores what the HOST Huffman routine makes of each chunk, by OpenEXR's rule"""
    def hook(c, _):
        raw = rep_chunks[c]
        z = K.deflate_huffman_host(R.predict(raw))
        return z if len(z) < len(raw) else raw
    return hook


def check_file(tmp_path, data, img, pixel_type, compression, encoder, reverse=False):
    """the file against the reader, the reference's chunk table, zlib and the encoder's reference bytes; returns the coded flags"""
    want_file, rep = ref_file(tmp_path / "ref.exr", img, pixel_type, compression, reverse)
    path = str(tmp_path / "got.exr")
    with open(path, "wb") as f:
        f.write(data)
    values = img[..., ::-1] if reverse else img
    assert same_bits(EXR.read_exr(path).cpu().numpy(), stored_values(values, pixel_type))
    payload = EXR.read_payload(path)
    lines = R.LINES[COMPS[compression]]
    assert payload.header.n_chunks == len(rep["chunks"]) and payload.header.lines == lines
    assert payload.header.row_bytes == rep["row_bytes"] and payload.header.compression == COMPS[compression]
    assert payload.offsets.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in rep["chunks"]])]).tolist()
    coded = []
    for c, ((y, stored), raw) in enumerate(zip(file_chunks(data, rep), rep["chunks"])):
        assert y == c * lines
        if len(stored) == len(raw):
            assert stored == raw
            coded.append(False)
        else:
            assert len(stored) < len(raw) and zlib.decompress(stored) == R.predict(raw), c
            coded.append(True)
    assert payload.coded.tolist() == [int(v) for v in coded]
    if encoder == "host":
        assert coded == rep["coded"] and data == want_file                 # zlib.compress at its default level on both sides
    else:
        hooked, _ = ref_file(tmp_path / "hook.exr", img, pixel_type, compression, reverse, chunk_hook=huffman_hook(rep["chunks"]))
        assert data == hooked                                               # the device bytes are the host routine's
    return coded


@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("compression", ["zips", "zip"])
def test_noisy_half_ramp_is_coded_everywhere(tmp_path, compression, encoder):
    imgs = [noisy_ramp(33, 64, 1), noisy_ramp(17, 65, 2), noisy_ramp(33, 301, 3)]
    files = EXR.encode_exr([dev(a) for a in imgs], "half", compression, encoder)
    for img, data in zip(imgs, files):
        assert all(check_file(tmp_path, data, img, "half", compression, encoder))


@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("compression", ["zips", "zip"])
def test_white_noise_float_is_stored_raw(tmp_path, compression, encoder):
    imgs = [white_noise(33, 64, 4), white_noise(17, 7, 5)]
    files = EXR.encode_exr([dev(a) for a in imgs], "float", compression, encoder, saturate=False)
    for img, data in zip(imgs, files):
        assert not any(check_file(tmp_path, data, img, "float", compression, encoder))


@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("compression", ["zips", "zip"])
@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_mixed_files_and_wild_values(tmp_path, pixel_type, compression, encoder):
    """A FLOAT file whose upper rows are a noise-free ramp and whose lower rows are random bits has coded and raw chunks (a chunk is a
    group of whole rows, so a left / right split puts both kinds of data into every chunk: that file is checked for its bytes only).
    As HALF most of the random bits saturate or vanish, so nothing is claimed about which chunks shrink."""
    h, w = 49, 66
    ramp = noisy_ramp(h, w, 6) if pixel_type == "half" else np.round(noisy_ramp(h, w, 6) * 16) / 16
    noise = white_noise(h, w, 7)
    rows = np.where(np.arange(h)[:, None, None] < 32, ramp, noise).astype(np.float32)
    cols = np.where(np.arange(w)[None, :, None] < w // 2, ramp, noise).astype(np.float32)
    wild = wild_image(33, 65, 8)
    files = EXR.encode_exr([dev(rows), dev(cols), dev(wild)], pixel_type, compression, encoder, reverse_channels=True)
    coded = check_file(tmp_path, files[0], rows, pixel_type, compression, encoder, reverse=True)
    if pixel_type == "float":
        assert any(coded) and not all(coded)
    check_file(tmp_path, files[1], cols, pixel_type, compression, encoder, reverse=True)
    check_file(tmp_path, files[2], wild, pixel_type, compression, encoder, reverse=True)


def test_write_exr_and_host_arrays(tmp_path):
    img = noisy_ramp(17, 65, 9)
    paths = [str(tmp_path / n) for n in ("a.exr", "b.exr", "c.exr")]
    EXR.write_exr(paths[0], dev(img))
    EXR.write_exr(paths[1], img)                                             # a float32 host array is uploaded
    EXR.write_exr(paths[2], dev(img), encoder="device", pixel_type="float", compression="zips")
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read() == ref_file(tmp_path / "r.exr", img, "half", "zip")[0]
    assert same_bits(EXR.read_exr(paths[0]).cpu().numpy(), R.half_values(img)) and same_bits(EXR.read_exr(paths[2]).cpu().numpy(), img)


def test_refusals(tmp_path):
    t = dev(noisy_ramp(4, 5, 1))
    for comp in ("rle", "piz", "pxr24", "b44", "dwaa"):
        with pytest.raises(ValueError, match=comp.upper()):
            EXR.encode_exr(t, compression=comp)
    with pytest.raises(ValueError, match="compression"):
        EXR.encode_exr(t, compression=3)
    with pytest.raises(ValueError, match="uint"):
        EXR.encode_exr(t, pixel_type="uint")
    with pytest.raises(ValueError, match="gpu"):
        EXR.encode_exr(t, encoder="gpu")
    for bad in (t.double(), t.half(), t[..., :2], t.reshape(-1), torch.zeros((2, 3, 4, 3, 3), device="cuda"), t.to(torch.uint8)):
        with pytest.raises(ValueError):
            EXR.encode_exr(bad)
    with pytest.raises(ValueError):
        EXR.encode_exr(np.zeros((4, 5, 3), dtype=np.float64))
    with pytest.raises(ValueError):
        EXR.encode_exr([])
    with pytest.raises(ValueError):
        EXR.write_exr(str(tmp_path / "x.exr"), t[None])
    with pytest.raises(ValueError, match="output_format"):
        IO.HdrReconstructor(lambda x: x).reconstruct_file("a.jpg", "b.exr", output_format="tiff")


# ---- file loop ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recon():
    from oracle import nets
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    ms = {k: getattr(pkg, mods[k]).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), 60 + i)) for i, k in enumerate(mods)}
    return IO.HdrReconstructor(pkg.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"]))


@pytest.fixture(scope="module")
def sources(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("exr_loop")
    rng = np.random.default_rng(12)
    paths = []
    for i, (h, w) in enumerate(((64, 96), (64, 64), (40, 50))):                     # two with a side that is no multiple of 64
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack((xx * 255.0 / w, yy * 255.0 / h, np.full((h, w), 90.0)), axis=-1)
        base[: h // 4, : w // 4] = 255.0                                            # a saturated corner
        paths.append(str(root / ("in%d.png" % i)))
        Image.fromarray(np.clip(base + rng.normal(0, 3, base.shape), 0, 255).astype(np.uint8)).save(paths[-1])
    return root, paths


@pytest.mark.parametrize("pixel_type", ["float", "half"])
def test_file_loop_writes_the_device_estimate(recon, sources, pixel_type):
    root, paths = sources
    out = str(root / ("single_%s.exr" % pixel_type))
    recon.reconstruct_file(paths[0], out, output_format="exr", exr_options=dict(pixel_type=pixel_type))
    want = recon.reconstruct_device(IO.read_ldr(paths[0])).cpu().numpy()[..., ::-1]         # the network's channel 0 is the file's blue
    assert want.shape == (64, 96, 3)
    assert same_bits(EXR.read_exr(out).cpu().numpy(), stored_values(want, pixel_type))
    assert EXR.read_header(out).compression == R.ZIP


def test_file_loop_defaults_still_write_radiance(recon, sources):
    root, paths = sources
    out = str(root / "default.hdr")
    recon.reconstruct_file(paths[0], out)
    rgbe = K.rgbe_encode(recon.reconstruct_device(IO.read_ldr(paths[0])), reverse_channels=True).cpu().numpy()
    want = str(root / "want.hdr")
    IO.write_hdr(want, rgbe)
    assert open(out, "rb").read() == open(want, "rb").read() and open(out, "rb").read().startswith(b"#?RADIANCE")


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_reconstruct_files_equals_single_calls(recon, sources, encoder):
    root, paths = sources
    opts = dict(pixel_type="float", compression="zips")
    batch = [str(root / ("batch_%s_%d.exr" % (encoder, i))) for i in range(3)]
    recon.reconstruct_files(paths, batch, encoder=encoder, output_format="exr", exr_options=opts)
    for i, (src, got) in enumerate(zip(paths, batch)):
        one = str(root / ("one_%s_%d.exr" % (encoder, i)))
        recon.reconstruct_file(src, one, encoder=encoder, output_format="exr", exr_options=opts)
        assert open(got, "rb").read() == open(one, "rb").read()
    d = root / ("dir_" + encoder)
    d.mkdir()
    written = recon.reconstruct_dir(str(root), str(d), pattern="in*.png", verbose=False, encoder=encoder, group=2, output_format="exr",
                                    exr_options=opts)
    assert [p.split("/")[-1] for p in written] == ["in0.exr", "in1.exr", "in2.exr"]
    assert [open(p, "rb").read() for p in written] == [open(p, "rb").read() for p in batch]
