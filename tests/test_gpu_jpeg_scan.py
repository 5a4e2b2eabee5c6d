"""The JPEG scan preparation on the device (csrc/jpeg_scan.hip: K.jpeg_scan / K.jpeg_compact, jpeg.plan_device, unstuff="device",
decoder="device_scan") against its host twin byte for byte, against the host route it replaces (jpeg.plan), and against PIL's pixels.
The corpus and the host twin are judged on the CPU in tests/test_jpeg_scan_host.py."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref
import jpeg_scan_ref as R
from test_gpu_jpeg import CASES, GROUPS, _folder, _noise_file
from test_jpeg_scan_host import CORPUS, J, compare, pack, seg_dwords

pytestmark = pytest.mark.gpu

# three batches of a hundred-odd regions each, lengths of 0 .. 3 tiles mixed (so that the regions start in every 16-byte class of a
# tile), the region of 300 tiles -- two workgroups of the cross-tile prefix sum -- in the middle of the first; and one single image
BATCHES = {"every_third_%d" % k: CORPUS[k::3] for k in range(3)}
BATCHES["every_third_0"] = BATCHES["every_third_0"][:50] + [CORPUS[-1]] + BATCHES["every_third_0"][50:]
BATCHES["every_third_%d" % ((len(CORPUS) - 1) % 3)].pop()
BATCHES["single_image"] = [c for c in CORPUS if c[0] == "stuffing_then_restart_across_T"]
BATCHES["single_long_image"] = [CORPUS[-1]]
BATCHES["single_empty_image"] = [c for c in CORPUS if c[0] == "length_0"]       # no tile at all


def test_the_batches_hold_the_corpus():
    names = sorted(c[0] for k, b in BATCHES.items() if k.startswith("every") for c in b)
    assert names == sorted(c[0] for c in CORPUS) and len(BATCHES["single_image"]) == 1
    _, desc = pack(BATCHES["every_third_1"])
    assert len(set((desc["offset"] % J.SCAN_TILE).tolist())) > 50


@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_corpus_batches_equal_the_host_twin(shdr, batch):
    K = shdr._ops
    cases = BATCHES[batch]
    src, desc = pack(cases)
    want_arena, dwords = seg_dwords(cases)
    h_report, h_bounds, h_arena = K.jpeg_scan_host(src, desc, dwords, 1, want_arena.size)
    src_dev = torch.from_numpy(src).cuda()
    result, ws, desc_dev = K.jpeg_scan(src_dev, desc)
    back = result.cpu().numpy()
    assert np.array_equal(back[:h_report.size], h_report), "report"
    assert np.array_equal(back[h_report.size:].view(np.int64), h_bounds), "bounds"
    arena = K.jpeg_compact(src_dev, desc, desc_dev, result, ws, torch.from_numpy(dwords).cuda(), 1, want_arena.size)
    assert np.array_equal(arena.cpu().numpy(), h_arena), "arena"
    compare(cases, desc, back[:h_report.size].view(J.SCAN_REPORT_DTYPE), back[h_report.size:].view(np.int64), arena.cpu().numpy())
    ms = []
    again, _, _ = K.jpeg_scan(src_dev, desc, desc_dev, stage_ms=ms)        # the timed form, and the same bits twice
    assert torch.equal(again, result) and len(ms) == 1 and 0.0 < ms[0] < 1000.0


def test_library_refuses_bad_descriptors(shdr):
    K = shdr._ops
    src, desc = pack(CORPUS[:3])
    src_dev = torch.from_numpy(src).cuda()
    bad = desc.copy()
    bad["length"][2] = src.size                                           # runs past the source buffer
    with pytest.raises(RuntimeError, match="image 2"):
        K.jpeg_scan(src_dev, bad)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        K.jpeg_scan(torch.from_numpy(np.concatenate([[0], src]).astype(np.uint8)).cuda()[1:], desc)


RESTART_FILES = [("256x384-420-rst%d" % b, _noise_file(restart_marker_blocks=b)) for b in (1, 5, 24)]
FILE_GROUPS = {g: [(n, d) for n, d in CASES if n.rsplit("-", 1)[0] == g] for g in GROUPS}
FILE_GROUPS["restart-files"] = RESTART_FILES
FILE_GROUPS["noise-256x384"] = [("256x384-420-noise", _noise_file())]
by_name = dict(CASES)
FILE_GROUPS["mixed-layouts-and-sizes"] = [(n, by_name[n]) for n in ("1x1-420-q75", "47x33-422-q100", "23x17-grey-q30", "47x33-444-rst3",
                                                                    "40x64-420-optimize", "16x16-444-q75")] + RESTART_FILES[1:2]


@pytest.mark.parametrize("group", sorted(FILE_GROUPS))
def test_plan_device_equals_plan_and_pixels_equal_pil(shdr, group):
    jpeg = shdr.jpeg
    files = [d for _, d in FILE_GROUPS[group]]
    want = jpeg.plan(files)
    got = jpeg.plan_device(files)
    assert got.data.is_cuda and got.data.dtype == torch.uint8 and np.array_equal(got.data.cpu().numpy(), want.data)
    for field in ("segs", "sub_seg", "images", "tables"):
        assert np.array_equal(getattr(got, field), getattr(want, field)), field
    assert (got.n_blocks, got.plane_bytes, got.out_bytes, got.subseq_bits) == (want.n_blocks, want.plane_bytes, want.out_bytes, want.subseq_bits)
    assert [h.scan_end for h in got.headers] == [h.scan_end for h in want.headers]
    host = jpeg.decode(files)
    dev = jpeg.decode(files, unstuff="device")
    for (name, data), a, b in zip(FILE_GROUPS[group], dev, host):
        assert torch.equal(a, b), name
        assert np.array_equal(a.cpu().numpy(), jpeg_ref.pil_rgb(data)), name


def test_other_subsequence_length_and_coefficients(shdr):
    jpeg = shdr.jpeg
    data = RESTART_FILES[1][1]
    want = jpeg.plan([data], 256)
    got = jpeg.plan_device([data], subseq_bits=256)
    assert np.array_equal(got.segs, want.segs) and np.array_equal(got.sub_seg, want.sub_seg)
    for a, b in zip(jpeg.decode_coefficients(data, unstuff="device"), jpeg.decode_coefficients(data)):
        assert torch.equal(a, b)
    d = jpeg.Decoded([data], unstuff="device")
    assert set(d.host_ms) == {"read_parse", "stage", "scan_launch", "scan_wait", "layout", "compact_launch", "upload"}
    assert all(v >= 0.0 for v in d.host_ms.values())
    with pytest.raises(ValueError, match="unstuff"):
        jpeg.decode([data], unstuff="gpu")


def test_exif_orientation_6(shdr, tmp_path):
    jpeg = shdr.jpeg
    exif = Image.Exif()
    exif[0x0112] = 6
    path = str(tmp_path / "o6.jpg")
    with open(path, "wb") as f:
        f.write(jpeg_ref.encode(jpeg_ref.content(3, 23, 17), "420", 90, exif=exif))
    want = torch.from_numpy(shdr.hdr_io.read_ldr(path))
    got = jpeg.decode([path], unstuff="device")[0]
    assert tuple(got.shape) == (17, 23, 3) and torch.equal(got.cpu(), want) and torch.equal(got, jpeg.decode([path])[0])
    assert torch.equal(jpeg.read_ldr_device(path, unstuff="device").cpu(), want)


def _damaged():
    """{kind: bytes}: files the host checks refuse after the header walk"""
    good = RESTART_FILES[1][1]
    hd = J.parse(good)
    first, fourth = int(hd.rst_offsets[0]), int(hd.rst_offsets[3])
    plain = by_name["40x64-420-q75"]
    ph = J.parse(plain)
    return {"cut inside its scan": plain[:(ph.scan_start + ph.scan_end) // 2],
            "cut after the SOS header": plain[:ph.scan_start],
            "a second scan": plain[:ph.scan_end] + b"\xff\xda\x00\x0c" + plain[ph.scan_end:],
            "another marker after the scan": plain[:ph.scan_end] + b"\xff\xe1\x00\x04ab" + plain[ph.scan_end:],
            "fill bytes in the scan": good[:first] + b"\xff" + good[first:],
            "one restart marker removed": good[:fourth] + good[fourth + 2:]}


DAMAGED = _damaged()


def _refusal(fn):
    with pytest.raises((J.Unsupported, J.CorruptJpeg)) as info:
        fn()
    return type(info.value), str(info.value)


@pytest.mark.parametrize("kind", sorted(DAMAGED))
def test_errors_are_those_of_the_host_route(shdr, kind, tmp_path):
    jpeg = shdr.jpeg
    bad = DAMAGED[kind]
    words = {"cut inside its scan": "no EOI marker", "cut after the SOS header": "no EOI marker", "a second scan": "several scans",
             "another marker after the scan": "marker FFE1 after", "fill bytes in the scan": "fill bytes",
             "one restart marker removed": "restart segments"}[kind]
    host = _refusal(lambda: jpeg.decode([bad]))
    assert words in host[1]
    assert _refusal(lambda: jpeg.decode([bad], unstuff="device")) == host
    path = str(tmp_path / "bad.jpg")
    with open(path, "wb") as f:
        f.write(bad)
    good, other = by_name["16x16-420-q75"], by_name["23x17-grey-q30"]
    host = _refusal(lambda: jpeg.decode([good, path, other]))
    assert "bad.jpg" in host[1] and words in host[1]
    assert _refusal(lambda: jpeg.decode([good, path, other], unstuff="device")) == host
    if issubclass(host[0], jpeg.Unsupported):                             # out of scope: PIL's job, as with unstuff="host"
        for unstuff in ("host", "device"):
            try:
                want = shdr.hdr_io.read_ldr(path)
            except Exception:
                break                                                     # (PIL refuses the file too)
            assert np.array_equal(jpeg.read_ldr_device(path, unstuff=unstuff).cpu().numpy(), want)


def test_first_bad_item_is_named_whatever_its_fault(shdr):
    """the host route stops at the first bad item; a later file that is not even a JPEG does not change which one is named"""
    jpeg = shdr.jpeg
    items = [by_name["16x16-420-q75"], DAMAGED["cut inside its scan"], b"not a jpeg at all", by_name["8x8-444-q75"]]
    assert _refusal(lambda: jpeg.decode(items, unstuff="device")) == _refusal(lambda: jpeg.decode(items))
    items = [by_name["16x16-420-q75"], b"\xff\xd8 no more", DAMAGED["cut inside its scan"]]
    assert _refusal(lambda: jpeg.decode(items, unstuff="device")) == _refusal(lambda: jpeg.decode(items))
    assert _refusal(lambda: jpeg.decode([b"PNG"], unstuff="device")) == _refusal(lambda: jpeg.decode([b"PNG"]))


def test_hdr_real_folder_device_scan(shdr, tmp_path):
    root = _folder(tmp_path, shdr)
    kw = dict(size=32, stride=16, seed=3, batch_size=4)
    a = shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="device", **kw)
    b = shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="device_scan", **kw)
    assert torch.equal(a.ldr_arena, b.ldr_arena) and a.shapes == b.shapes and a.candidates == b.candidates and len(a.candidates) > 0
    (la, ha), (lb, hb) = next(iter(a)), next(iter(b))
    assert torch.equal(la, lb) and torch.equal(ha, hb)
    with pytest.raises(ValueError, match="device_scan"):
        shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="cpu", **kw)
    # a file that only its scan puts out of scope (fill bytes): PIL reads it, the others still decode on the device
    path = os.path.join(root, "LDR_in", "01.jpg")
    ldr = shdr.hdr_io.read_ldr(path)
    data = jpeg_ref.encode(ldr, "444", 92, restart_marker_blocks=4)
    first = int(J.parse(data).rst_offsets[0])
    with open(path, "wb") as f:
        f.write(data[:first] + b"\xff" + data[first:])
    with pytest.raises(J.Unsupported, match="fill bytes"):
        J.plan([path])
    c = shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="device", **kw)
    d = shdr.hdr_real.HdrRealFolder(root, jpeg_decoder="device_scan", **kw)
    assert torch.equal(c.ldr_arena, d.ldr_arena) and torch.equal(c.ldr_arena, shdr.hdr_real.HdrRealFolder(root, **kw).ldr_arena)


def test_reconstruct_files_device_scan(shdr, tmp_path):
    from oracle import nets
    models = []
    for i, (k, mod) in enumerate(dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net",
                                      ref="refinement_net").items()):
        models.append(getattr(shdr, mod).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), 100 + i)))
    recon = shdr.hdr_io.HdrReconstructor(shdr.pipeline.Inference(*models))
    src = []
    for i, (layout, kw) in enumerate((("420", {}), ("444", dict(restart_marker_blocks=3)))):
        src.append(str(tmp_path / ("in%d.jpg" % i)))
        with open(src[-1], "wb") as f:
            f.write(jpeg_ref.encode(jpeg_ref.content(6 + i, 40, 56), layout, 90, **kw))
    out = {}
    for decoder in ("device", "device_scan"):
        dst = [str(tmp_path / ("%s%d.hdr" % (decoder, i))) for i in range(len(src))]
        recon.reconstruct_files(src, dst, decoder=decoder)
        out[decoder] = [open(p, "rb").read() for p in dst]
    assert out["device"] == out["device_scan"] and all(len(b) > 40 * 56 for b in out["device"])
    recon.reconstruct_file(src[0], str(tmp_path / "one.hdr"), decoder="device_scan")
    assert open(tmp_path / "one.hdr", "rb").read() == out["device"][0]
    for call in (lambda: recon.reconstruct_files(src, src, decoder="gpu"), lambda: recon.reconstruct_file(src[0], src[0], decoder="gpu")):
        with pytest.raises(ValueError, match="device_scan"):
            call()
