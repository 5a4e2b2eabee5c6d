"""The device PIZ encoder (K.piz_encode, csrc/piz_enc.hip) against its host twin (K.piz_encode_host, the same rules of csrc/piz.h, which
tests/test_piz_enc_host.py holds to tests/piz_ref.py byte for byte): stored bytes, offsets and coded flags of one mixed batch, gaps left
untouched, the same bytes on every run, the device decoder reading them back; PIZ files through exr.encode_exr (device against host
against piz_ref.write_exr, file byte for file byte), read back by both readers; the file loop; the refusals."""
import importlib

import numpy as np
import pytest
import torch

import exr_ref as R
import piz_enc_cases
import piz_ref

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
K, EXR, IO = pkg._ops, pkg.exr, pkg.hdr_io

FILL = 0xA5
CHUNKS = piz_enc_cases.chunks()
PTYPES = {"half": R.HALF, "float": R.FLOAT}


def tables(chunks):
    off = np.concatenate([[0], np.cumsum([len(c.raw) for c in chunks])]).astype(np.int64)
    geom, words = np.zeros((len(chunks), 4), dtype=np.int32), []
    for i, c in enumerate(chunks):
        geom[i] = (c.width, c.rows, len(words), len(c.words))
        words += list(c.words)
    return off, geom, words


@pytest.fixture(scope="module")
def batch():
    """the chunks on the device, their tables, and what the host twin stores for each: (bytes, coded)"""
    off, geom, words = tables(CHUNKS)
    planar = torch.from_numpy(np.frombuffer(b"".join(c.raw for c in CHUNKS), dtype=np.uint8).copy()).cuda()
    want = []
    for c in CHUNKS:
        z = K.piz_encode_host(c.raw, c.width, c.rows, c.words)
        want.append((z, 1) if len(z) < len(c.raw) else (c.raw, 0))
    return planar, off, geom, words, want


def run(batch, pad=0, front=0):
    """one K.piz_encode call into a buffer filled with FILL: (host bytes of the buffer, out_offsets, coded)"""
    planar, off, geom, words, _ = batch
    out = torch.full((front + int(off[-1]) + pad * len(CHUNKS) + 64,), FILL, dtype=torch.uint8, device="cuda")
    got, out_offsets, coded = K.piz_encode(planar, off, geom, words, pad=pad, front=front, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy(), out_offsets.cpu().numpy(), coded.cpu().numpy()


@pytest.mark.parametrize("pad,front", [(0, 0), (8, 8 * len(CHUNKS)), (3, 5)])
def test_batch_equals_the_host_twin(batch, pad, front):
    want = batch[4]
    data, out_offsets, coded = run(batch, pad, front)
    sizes = [pad + len(z) for z, _ in want]
    assert out_offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert coded.tolist() == [flag for _, flag in want]
    assert (data[:front] == FILL).all() and (data[front + out_offsets[-1]:] == FILL).all()
    for i, (c, (z, _)) in enumerate(zip(CHUNKS, want)):
        at = front + int(out_offsets[i])
        assert (data[at:at + pad] == FILL).all(), c.name
        assert data[at + pad:front + int(out_offsets[i + 1])].tobytes() == z, c.name
    names = [c.name for c in CHUNKS]
    for name, flag in (("shuffled_100x32", 0), ("one_pixel", 0), ("ordered_100x32", 1), ("stretches_65x32", 1)):
        assert coded[names.index(name)] == flag, name              # the strictly-smaller rule, both ways


def test_two_runs_give_the_same_bytes(batch):
    a, b = run(batch, 8, 16), run(batch, 8, 16)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_the_device_decoder_reads_it_back(batch):
    planar, off, geom, words, want = batch
    out, out_offsets, coded = K.piz_encode(planar, off, geom, words)
    dst, written, status = K.piz_decode(out, out_offsets.cpu().numpy(), off, geom, words, mode=coded)
    assert status.cpu().tolist() == [0] * len(CHUNKS)
    assert written.cpu().tolist() == np.diff(off).tolist()
    assert torch.equal(dst, planar)


def test_stage_times(batch):
    planar, off, geom, words, _ = batch
    ms = []
    stats = K.piz_encode(planar, off, geom, words, stage_ms=ms, stats=True)[3].cpu().numpy()
    assert len(ms) == K.PIZ_ENC_STAGES == len(K.PIZ_ENC_STAGE_NAMES) and all(t >= 0 for t in ms)
    # the symbols of every chunk's code: the values its sequence holds, and the run code
    used = [np.unique(piz_enc_cases.value_sequence(c.raw, c.width, c.rows, c.words)).size + 1 for c in CHUNKS]
    assert stats[:, 0].tolist() == used and (stats[:, 1] >= 0).all()


def test_shape_errors(batch):
    planar, off, geom, words, _ = batch
    bad = geom.copy()
    bad[3, 1] = 33
    with pytest.raises(RuntimeError, match="rows"):
        K.piz_encode(planar, off, bad, words)
    bad = off.copy()
    bad[1:] += 2
    with pytest.raises((RuntimeError, ValueError)):
        K.piz_encode(planar, bad, geom, words)
    with pytest.raises(ValueError):
        K.piz_encode(planar, off, geom[:-1], words)


# ---- files --------------------------------------------------------------------------------------------------------------------
def smooth_noisy(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack((1.0 + xx / w + yy / h, 0.5 + 0.25 * xx / w + 0.1 * yy / h, 2.0 + 3.0 * (xx + yy) / (h + w)), axis=-1)
    return (base * (1.0 + 0.02 * rng.standard_normal(base.shape))).astype(np.float32)


IMAGES = [smooth_noisy(40, 64, 1), smooth_noisy(33, 47, 2), smooth_noisy(1, 1, 3)]


@pytest.mark.parametrize("pixel_type", ["half", "float"])
def test_files(tmp_path, pixel_type):
    dev = [torch.from_numpy(x).cuda() for x in IMAGES]
    on_device = EXR.encode_exr(dev, pixel_type=pixel_type, compression="piz", piz="device")
    on_host = EXR.encode_exr(dev, pixel_type=pixel_type, compression="piz", piz="host", encoder="device_lz")      # encoder plays no part
    assert on_device == on_host
    for i, (img, data) in enumerate(zip(IMAGES, on_device)):
        ref = str(tmp_path / ("ref%d.exr" % i))
        with np.errstate(over="ignore"):
            piz_ref.write_exr(ref, {"RGB"[k]: (img[..., k], PTYPES[pixel_type]) for k in range(3)})
        assert data == open(ref, "rb").read(), i
        path = str(tmp_path / ("got%d.exr" % i))
        EXR.write_exr(path, dev[i], pixel_type=pixel_type, compression="piz", piz="device")
        assert open(path, "rb").read() == data
        want = img if pixel_type == "float" else img.astype(np.float16).astype(np.float32)
        for piz in ("host", "device"):
            got = EXR.read_exr(path, piz=piz).cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (i, piz)


def test_file_loop(tmp_path):
    from PIL import Image
    from oracle import nets
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    ms = {k: getattr(pkg, mods[k]).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), 60 + i)) for i, k in enumerate(mods)}
    recon = IO.HdrReconstructor(pkg.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"]))
    h, w = 40, 50
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack((xx * 255.0 / w, yy * 255.0 / h, np.full((h, w), 90.0)), axis=-1)
    src, out = str(tmp_path / "in.png"), str(tmp_path / "out.exr")
    Image.fromarray(np.clip(base + np.random.default_rng(4).normal(0, 3, base.shape), 0, 255).astype(np.uint8)).save(src)
    recon.reconstruct_file(src, out, output_format="exr", exr_options=dict(compression="piz", piz="device"))
    want = recon.reconstruct_device(IO.read_ldr(src)).cpu().numpy()[..., ::-1]           # the network's channel 0 is the file's blue
    with np.errstate(over="ignore", invalid="ignore"):
        want = R.half_values(np.where(np.isfinite(want), np.clip(want, -65504.0, 65504.0), want))
    got = EXR.read_exr(out, piz="host").cpu().numpy()
    assert got.shape == (h, w, 3) and np.array_equal(got.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))
    assert open(out, "rb").read()[:4] == b"\x76\x2f\x31\x01" and EXR.read_item(out, "host", "host").header.compression == EXR.PIZ_COMPRESSION


def test_refusals():
    t = torch.from_numpy(IMAGES[1]).cuda()
    with pytest.raises(ValueError, match="PIZ compression is not supported"):
        EXR.encode_exr(t, compression="piz")
    with pytest.raises(ValueError, match="gpu"):
        EXR.encode_exr(t, compression="piz", piz="gpu")
    with pytest.raises(ValueError, match="piz"):
        EXR.encode_exr(t, compression="zip", piz="device")
    with pytest.raises(ValueError, match="piz"):
        EXR.encode_exr(t, compression="none", piz="host")
