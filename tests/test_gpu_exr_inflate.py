"""OpenEXR files whose ZIP / ZIPS chunks the device inflates (exr.read_stored, exr.upload_batch, inflate="device") against the host
route (zlib): the same planes, pixels, arenas and means, bit for bit, and the same refusals."""
import importlib
import os
import zlib

import numpy as np
import pytest
import torch

import exr_ref as X

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
E = pkg.exr
D = pkg.dataset
IO = pkg.hdr_io
HR = pkg.hdr_real

WIDTHS = (1, 7, 64, 100)
HEIGHTS = (1, 15, 16, 17, 33)


def _plane(rng, h, w, noisy_rows=()):
    """smooth values (chunks that compress) with rows of noise (FLOAT rows of noise do not: ZIPS stores them raw)"""
    img = (0.5 + np.add.outer(np.arange(h), np.arange(w)) / 64.0).astype(np.float32)
    for y in noisy_rows:
        if y < h:
            img[y] = rng.normal(0.0, 1e3, w)
    return img


def write_files(d):
    """ZIP and ZIPS, HALF and FLOAT, every width and height of the lists, an extra A channel, DECREASING_Y, noisy FLOAT rows"""
    rng = np.random.default_rng(41)
    paths, k = [], 0
    for comp in (X.ZIP, X.ZIPS):
        for w in WIDTHS:
            for h in HEIGHTS:
                t = (X.HALF, X.FLOAT)[k % 2]
                ch = {c: (_plane(rng, h, w, noisy_rows=(1, 16) if t == X.FLOAT else ()), t) for c in "RGB"}
                if k % 3 == 0:
                    ch["A"] = (_plane(rng, h, w), (X.HALF, X.FLOAT, X.UINT)[(k // 3) % 3])
                path = os.path.join(d, "f%02d_c%d_%dx%d.exr" % (k, comp, h, w))
                info = X.write_exr(path, ch, comp, (X.INC, X.DEC)[(k // 2) % 2], origin=(k - 3, 2 - k))
                paths.append((path, info))
                k += 1
    return paths


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return write_files(str(tmp_path_factory.mktemp("exr_inflate")))


def test_the_files_hold_coded_and_raw_chunks(files):
    coded = [c for _, info in files for c in info["coded"]]
    assert coded.count(True) > 100 and coded.count(False) > 10
    assert any(True in info["coded"] and False in info["coded"] for _, info in files)        # raw beside coded in one file


def test_read_stored_makes_the_host_routes_checks_and_inflates_nothing(files):
    for path, info in files:
        s, p = E.read_stored(path), E.read_payload(path)
        assert isinstance(s, E.Stored) and s.path == path and s.header == p.header
        assert np.array_equal(s.offsets, p.offsets) and np.array_equal(s.mode, p.coded)
        assert s.mode.tolist() == [int(c) for c in info["coded"]]
        assert s.data.dtype == np.uint8 and s.data.size == s.src_offsets[-1] and s.src_offsets[0] == 0
        for c in range(s.header.n_chunks):
            stored = s.data[s.src_offsets[c]:s.src_offsets[c + 1]].tobytes()
            assert (X.unpredict(zlib.decompress(stored)) if s.mode[c] else stored) == info["chunks"][c]


def test_upload_batch_gives_the_planes_of_the_host_route(files):
    dev = torch.device("cuda")
    items = [E.read_stored(p) for p, _ in files]
    got = E.upload_batch(items, dev)
    assert len(got) == len(files)
    for (path, info), (planes, offsets) in zip(files, got):
        want_planes, want_offsets = E.upload(E.read_payload(path), dev)
        assert torch.equal(planes, want_planes) and torch.equal(offsets, want_offsets), path
        assert bytes(planes.cpu().numpy()) == b"".join(info["chunks"])


def test_upload_batch_of_one_file_and_of_a_mix_with_payloads(files, tmp_path):
    dev = torch.device("cuda")
    rng = np.random.default_rng(42)
    rle, none = str(tmp_path / "rle.exr"), str(tmp_path / "none.exr")
    X.write_exr(rle, {c: (_plane(rng, 20, 33), X.HALF) for c in "RGB"}, X.RLE)
    X.write_exr(none, {c: (_plane(rng, 5, 9), X.FLOAT) for c in "RGB"}, X.NONE)
    assert isinstance(E.read_stored(rle), E.Payload) and isinstance(E.read_stored(none), E.Payload)
    paths = [files[3][0], rle, files[20][0], none, files[0][0]]
    items = [E.read_stored(p) for p in paths]
    items[2] = E.read_payload(paths[2])                             # a ZIP file inflated on the host already
    for sub in ([items[0]], [items[1]], items):
        for it, (planes, offsets) in zip(sub, E.upload_batch(sub, dev)):
            want_planes, want_offsets = E.upload(E.read_payload(paths[items.index(it)]), dev)
            assert torch.equal(planes, want_planes) and torch.equal(offsets, want_offsets)
    assert E.upload_batch([], dev) == []


def test_read_exr_device_equals_host_bit_for_bit(files):
    for path, _ in files:
        a, b = E.read_exr(path), E.read_exr(path, inflate="device")
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), path


def test_files_of_the_device_encoder(tmp_path):
    rng = np.random.default_rng(43)
    imgs = [torch.from_numpy(np.abs(rng.normal(1.0, 0.5, (h, w, 3))).astype(np.float32)).cuda() for h, w in ((33, 100), (16, 7), (70, 64))]
    for comp in ("zip", "zips"):
        for ptype in ("half", "float"):
            for i, data in enumerate(E.encode_exr(imgs, ptype, comp, encoder="device")):
                path = str(tmp_path / ("%s_%s_%d.exr" % (comp, ptype, i)))
                with open(path, "wb") as f:
                    f.write(data)
                a, b = E.read_exr(path), E.read_exr(path, inflate="device")
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), path


def _flip_a_byte_in_chunk(src, dst, chunk):
    """a copy of the file with one byte inside the chunk's zlib stream changed (past its two header bytes)"""
    s = E.read_stored(src)
    assert s.mode[chunk] == 1
    with open(src, "rb") as f:
        data = bytearray(f.read())
    table = np.frombuffer(bytes(data), dtype="<u8", count=s.header.n_chunks, offset=s.header.table_offset)
    size = int(s.src_offsets[chunk + 1] - s.src_offsets[chunk])
    data[int(table[chunk]) + 8 + min(10, size - 5)] ^= 0x55
    with open(dst, "wb") as f:
        f.write(bytes(data))


def test_a_flipped_byte_names_the_file_and_the_chunk_under_both_routes(files, tmp_path):
    src = next(p for p, info in files if len(info["coded"]) >= 3 and info["coded"][2])
    bad = str(tmp_path / "flipped.exr")
    _flip_a_byte_in_chunk(src, bad, 2)
    with pytest.raises(ValueError, match=r"flipped\.exr: chunk 2: "):
        E.read_exr(bad)
    with pytest.raises(ValueError, match=r"flipped\.exr: chunk 2: inflate error: "):
        E.read_exr(bad, inflate="device")
    good = [E.read_stored(p) for p, _ in files[:3]]
    with pytest.raises(ValueError, match=r"flipped\.exr: chunk 2: inflate error: "):           # the second file of a batch
        E.upload_batch([good[0], E.read_stored(bad), good[1]], torch.device("cuda"))


def test_container_errors_keep_their_messages(files, tmp_path):
    src = files[0][0]
    with open(src, "rb") as f:
        data = f.read()
    cut = str(tmp_path / "cut.exr")
    with open(cut, "wb") as f:
        f.write(data[:-3])
    for read in (E.read_payload, E.read_stored):
        with pytest.raises(ValueError, match=r"cut\.exr: chunk \d+: size \d+ runs past the end of the file"):
            read(cut)
    with pytest.raises(ValueError, match="inflate must be 'host' or 'device'"):
        E.read_exr(src, inflate="gpu")
    with pytest.raises(ValueError, match="inflate must be 'host' or 'device'"):
        D.PatchHDRDataset(os.path.dirname(src), [os.path.basename(src)], True, exr_inflate="zlib")
    with pytest.raises(ValueError, match="inflate must be 'host' or 'device'"):
        HR.HdrRealFolder(str(tmp_path), exr_inflate=None)


@pytest.fixture(scope="module")
def training_dir(tmp_path_factory):
    """ZIP, ZIPS, RLE and NONE OpenEXR files and a Radiance file in one folder"""
    d = str(tmp_path_factory.mktemp("train"))
    rng = np.random.default_rng(44)
    names = []
    for i, (comp, t, (h, w)) in enumerate(((X.ZIP, X.HALF, (40, 64)), (X.ZIPS, X.FLOAT, (33, 100)), (X.RLE, X.HALF, (64, 48)),
                                           (X.NONE, X.HALF, (32, 32)), (X.ZIP, X.FLOAT, (100, 70)))):
        ch = {c: (np.abs(_plane(rng, h, w, noisy_rows=(3,) if t == X.FLOAT else ())), t) for c in "RGB"}
        names.append("e%d.exr" % i)
        X.write_exr(os.path.join(d, names[-1]), ch, comp)
    rgbe = rng.integers(1, 256, (48, 80, 4), dtype=np.uint8)
    rgbe[..., 3] = rng.integers(120, 136, (48, 80))
    IO.write_hdr(os.path.join(d, "r.hdr"), rgbe)
    return d, names[:2] + ["r.hdr"] + names[2:]


def test_patch_dataset_arena_and_means_are_the_same(training_dir):
    d, names = training_dir
    a = D.PatchHDRDataset(d, names, True)
    b = D.PatchHDRDataset(d, names, True, exr_inflate="device")
    assert a.shapes == b.shapes and torch.equal(a.arena.view(torch.int32), b.arena.view(torch.int32))
    assert torch.equal(a.means.view(torch.int32), b.means.view(torch.int32))
    assert set(b.load_seconds) == set(a.load_seconds) == {"host_decode", "device"}


def test_hdr_real_folder_arena_and_means_are_the_same(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(45)
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "HDR_gt"))
    os.makedirs(os.path.join(root, "LDR_in"))
    for i, (comp, t, (h, w)) in enumerate(((X.ZIP, X.HALF, (33, 47)), (X.ZIPS, X.FLOAT, (40, 52)), (X.RLE, X.HALF, (32, 32)), (None, None, (35, 40)))):
        if comp is None:
            rgbe = rng.integers(1, 256, (h, w, 4), dtype=np.uint8)
            rgbe[..., 3] = rng.integers(120, 136, (h, w))
            IO.write_hdr(os.path.join(root, "HDR_gt", "s%d.hdr" % i), rgbe)
        else:
            ch = {c: (np.abs(_plane(rng, h, w, noisy_rows=(2,) if t == X.FLOAT else ())), t) for c in "RGB"}
            X.write_exr(os.path.join(root, "HDR_gt", "s%d.exr" % i), ch, comp)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "LDR_in", "s%d.jpg" % i), quality=92)
    a = HR.HdrRealFolder(root, size=16, stride=8)
    b = HR.HdrRealFolder(root, size=16, stride=8, exr_inflate="device")
    assert a.files == b.files and a.shapes == b.shapes
    assert torch.equal(a.hdr_arena.view(torch.int32), b.hdr_arena.view(torch.int32)) and torch.equal(a.ldr_arena, b.ldr_arena)
    assert a.patches == b.patches and np.array_equal(a.means.view(np.uint32), b.means.view(np.uint32))
    assert set(b.load_seconds) == {"host_decode", "device"}
