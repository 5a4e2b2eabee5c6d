"""The device PIZ decoder (K.piz_decode, csrc/piz.hip) against its host twin (K.piz_decode_host, the same rules of csrc/piz.h, which
tests/test_piz_host.py holds to the tests' own codec): bytes, written counts and statuses are equal for every chunk; and PIZ files
through exr.upload_batch, read_exr and the dataset readers, device against host, bit for bit."""
import importlib
import os

import numpy as np
import pytest
import torch

import exr_ref as X
import piz_cases
import piz_ref

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
K = pkg._ops
E = pkg.exr
D = pkg.dataset
IO = pkg.hdr_io
HR = pkg.hdr_real

FILL = 0xA5


def run_batch(chunks, sub_bits=None, mode=None, slot_bytes=None, rounds=False):
    """chunks: [(data, width, rows, words)] -> (slots as bytes, written, status[, rounds]) of one K.piz_decode call into a buffer
    filled with FILL; slot_bytes: the slots' sizes if not the shapes'"""
    n = len(chunks)
    src = np.frombuffer(b"".join(c[0] for c in chunks), dtype=np.uint8)
    src_off = np.concatenate([[0], np.cumsum([len(c[0]) for c in chunks])]).astype(np.int64)
    sizes = slot_bytes or [2 * c[1] * c[2] * sum(c[3]) for c in chunks]
    dst_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    geom, words = np.zeros((n, 4), dtype=np.int32), []
    for i, (_, width, rows, w) in enumerate(chunks):
        geom[i] = (width, rows, len(words), len(w))
        words += list(w)
    dst = torch.full((int(dst_off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    out = K.piz_decode(torch.from_numpy(src.copy()).cuda(), src_off, dst_off, geom, words, sub_bits=sub_bits, dst=dst, rounds=rounds,
                       mode=None if mode is None else torch.tensor(mode, dtype=torch.uint8, device="cuda"))
    host = out[0].cpu().numpy().tobytes()
    slots = [host[dst_off[i]:dst_off[i + 1]] for i in range(n)]
    return (slots, out[1].cpu().tolist(), out[2].cpu().tolist()) + ((out[3].cpu().tolist(),) if rounds else ())


def host_twin(chunks):
    """what the host decoder makes of the same chunks and the same filled slots"""
    slots, written, status = [], [], []
    for data, width, rows, words in chunks:
        slot = np.full(2 * width * rows * sum(words), FILL, dtype=np.uint8)
        _, st = K.piz_decode_host(data, width, rows, words, out=slot)
        slots.append(slot.tobytes())
        status.append(st)
        written.append(slot.size if st == 0 else 0)
    return slots, written, status


@pytest.fixture(scope="module")
def matrix():
    chunks = [(c.data, c.width, c.rows, c.words) for c in piz_cases.cases()]
    return chunks, host_twin(chunks)


@pytest.mark.parametrize("sub_bits", [None, K.PIZ_MIN_SUB_BITS, 1024, 4096])
def test_matrix_equals_the_host_twin(matrix, sub_bits):
    # the smallest subsequences put hundreds of them, and so every carry between rounds, into chunks of a few hundred bytes
    chunks, (slots, written, status) = matrix
    got = run_batch(chunks, sub_bits)
    names = [c.name for c in piz_cases.cases()]
    assert got[2] == status == [0] * len(chunks), [(n, K.piz_reason(s)) for n, s in zip(names, got[2]) if s]
    assert got[1] == written
    for name, a, b, c in zip(names, got[0], slots, piz_cases.cases()):
        assert a == b, name
        assert c.raw is None or a == c.raw, name


def test_rounds_are_counted_and_small_subsequences_need_more(matrix):
    chunks, _ = matrix
    stats = np.asarray(run_batch(chunks, K.PIZ_MIN_SUB_BITS, rounds=True)[3])
    big, small = [r[0] for r in run_batch(chunks, 4096, rounds=True)[3]], stats[:, 0].tolist()
    assert stats.shape == (len(chunks), K.PIZ_ROUND_STATS)
    for c, row in zip(piz_cases.cases(), stats):                          # round 0 decodes every subsequence, later rounds fewer,
        n_bits = 8 * len(c.data)                                          # the last round nothing
        assert 1 <= row[1] <= -(-n_bits // K.PIZ_MIN_SUB_BITS) and all(row[1] > v for v in row[2:]), c.name
        assert row[min(row[0], K.PIZ_ROUND_STATS - 1)] == 0 or row[0] >= K.PIZ_ROUND_STATS, c.name
    assert min(big) >= 2 and min(small) >= 2                            # the first round, and the one that finds nothing changed
    assert max(small) >= 3 and sum(small) >= sum(big)                   # a token that straddles a border moves the next start


def test_damaged_chunks_among_good_ones():
    # every truncation and single-bit flip of one small chunk and every seventh of another, each between two good chunks
    a, b = piz_cases.small_cases()
    good = (a.data, a.width, a.rows, a.words)
    chunks = []
    for c, step in ((b, 1), (a, 7)):
        for k, (_, data) in enumerate(piz_cases.mutations(c.data)):
            if k % step == 0:
                chunks += [good, (data, c.width, c.rows, c.words)]
    chunks.append(good)
    slots, written, status = host_twin(chunks)
    assert status[0] == 0 and 0 < sum(1 for s in status if s) < len(status) and len(set(status)) >= 8
    for sub_bits in (None, K.PIZ_MIN_SUB_BITS):
        got = run_batch(chunks, sub_bits)
        assert got[2] == status
        assert got[1] == written
        assert got[0] == slots                                           # good neighbours intact, refused slots untouched


def test_batch_statuses_raw_chunks_and_bad_tables():
    a, b = piz_cases.small_cases()
    raw = bytes(range(36))
    chunks = [(a.data, a.width, a.rows, a.words), (raw, 3, 2, (1, 2)), (raw[:35], 3, 2, (1, 2)), (b.data, b.width, b.rows, b.words),
              (b.data, b.width, b.rows, b.words)]
    slots, written, status = run_batch(chunks, mode=[1, 0, 0, 7, 1])
    assert status == [0, 0, 15, 16, 0] and written == [36, 36, 0, 0, 18]
    assert slots[1] == raw and slots[2] == bytes([FILL]) * 36 and slots[3] == bytes([FILL]) * 18
    assert slots[0] == a.raw and slots[4] == piz_ref.decode_chunk(b.data, b.width, b.rows, b.words)
    with pytest.raises(RuntimeError, match="its slot has 20 bytes, its shape holds 18"):
        run_batch(chunks[3:], slot_bytes=[20, 18])
    with pytest.raises(RuntimeError, match="sub_bits must be 128"):
        run_batch(chunks[:1], sub_bits=64)
    with pytest.raises(RuntimeError, match="width 3, rows 33"):
        run_batch([(a.data, 3, 33, (1,))])


# ---- files ------------------------------------------------------------------------------------------------------------------------
def _plane(h, w, k):
    y, x = np.mgrid[0:h, 0:w]
    return np.exp(((x * (k + 1) + y * 3) % 64) / 16.0 - 2.0).astype(np.float32) * (k + 1)


def _channels(h, w, t=X.HALF, extra=()):
    ch = {n: (X.half_values(_plane(h, w, k)) if t == X.HALF else np.round(_plane(h, w, k) * 64) / 64, t) for k, n in enumerate("RGB")}
    for name, et in extra:
        ch[name] = ((np.arange(h * w).reshape(h, w) // 8 % 9).astype(np.uint32 if et == X.UINT else np.float32), et)
    return ch


@pytest.fixture(scope="module")
def piz_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("piz"))
    specs = ((70, 37, X.HALF, (), X.INC, (0, 0)), (33, 100, X.FLOAT, (), X.DEC, (-5, 9)), (64, 48, X.HALF, (("A", X.HALF), ("Z", X.FLOAT)), X.INC, (3, -40)),
             (32, 9, X.HALF, (("Z", X.UINT),), X.DEC, (0, 0)), (5, 2, X.HALF, (), X.INC, (0, 0)))
    out = []
    for i, (h, w, t, extra, order, origin) in enumerate(specs):
        path = os.path.join(d, "p%d.exr" % i)
        out.append((path, piz_ref.write_exr(path, _channels(h, w, t, extra), line_order=order, origin=origin)))
    assert sum(c for _, info in out for c in info["coded"]) >= 4 and not all(c for _, info in out for c in info["coded"])
    return out


def test_upload_batch_over_zip_rle_and_piz_files(piz_files, tmp_path):
    dev = torch.device("cuda")
    zip_path, rle_path = str(tmp_path / "z.exr"), str(tmp_path / "r.exr")
    zi = X.write_exr(zip_path, _channels(40, 33), X.ZIP)
    ri = X.write_exr(rle_path, _channels(20, 65, X.FLOAT), X.RLE)
    paths = [piz_files[0][0], zip_path, piz_files[2][0], rle_path, piz_files[4][0]]
    infos = [piz_files[0][1], zi, piz_files[2][1], ri, piz_files[4][1]]
    items = [E.read_item(p, "device", "device") for p in paths]
    assert [type(it).__name__ for it in items] == ["Stored", "Stored", "Stored", "Payload", "Stored"]
    for (planes, offsets), path, info in zip(E.upload_batch(items, dev), paths, infos):
        want_planes, want_offsets = E.upload(E.read_item(path, "host", "host"), dev)
        assert torch.equal(planes, want_planes) and torch.equal(offsets, want_offsets), path
        assert bytes(planes.cpu().numpy()) == b"".join(info["chunks"]), path


def test_read_exr_device_equals_host_equals_source(piz_files):
    for path, _ in piz_files:
        a, b = E.read_exr(path, piz="host"), E.read_exr(path, piz="device")
        assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), path
        with pytest.raises(ValueError, match="PIZ compression is not supported"):
            E.read_exr(path)
    h, w = 70, 37
    want = np.stack([X.half_values(_plane(h, w, k)) for k in range(3)], axis=-1)
    assert np.array_equal(E.read_exr(piz_files[0][0], piz="device").cpu().numpy(), want)


def test_a_damaged_chunk_names_the_file_and_the_chunk(piz_files, tmp_path):
    bad = str(tmp_path / "bad.exr")
    piz_ref.write_exr(bad, _channels(70, 37), chunk_hook=lambda c, s: s[:len(s) // 2] if c == 1 else s)
    with pytest.raises(ValueError, match=r"bad\.exr: chunk 1: PIZ error: "):
        E.read_exr(bad, piz="host")
    with pytest.raises(ValueError, match=r"bad\.exr: chunk 1: PIZ error: "):
        E.read_exr(bad, piz="device")
    good = E.read_stored(piz_files[0][0], piz="device")
    with pytest.raises(ValueError, match=r"bad\.exr: chunk 1: PIZ error: "):
        E.upload_batch([good, E.read_stored(bad, piz="device"), good], torch.device("cuda"))


def _training_dir(d):
    names = []
    for i, (comp, t, (h, w)) in enumerate((("piz", X.HALF, (40, 64)), (X.ZIPS, X.FLOAT, (33, 100)), (X.RLE, X.HALF, (64, 48)),
                                           ("piz", X.FLOAT, (100, 70)), (X.ZIP, X.HALF, (32, 32)))):
        names.append("e%d.exr" % i)
        if comp == "piz":
            piz_ref.write_exr(os.path.join(d, names[-1]), _channels(h, w, t))
        else:
            X.write_exr(os.path.join(d, names[-1]), _channels(h, w, t), comp)
    return names


def test_patch_dataset_arena_and_means_are_the_same(tmp_path):
    d = str(tmp_path)
    names = _training_dir(d)
    rng = np.random.default_rng(44)
    rgbe = rng.integers(1, 256, (48, 80, 4), dtype=np.uint8)
    rgbe[..., 3] = rng.integers(120, 136, (48, 80))
    IO.write_hdr(os.path.join(d, "r.hdr"), rgbe)
    names = names[:2] + ["r.hdr"] + names[2:]
    with pytest.raises(ValueError, match="PIZ compression is not supported"):
        D.PatchHDRDataset(d, names, True)
    a = D.PatchHDRDataset(d, names, True, exr_piz="host")
    for kw in (dict(exr_piz="device"), dict(exr_piz="device", exr_inflate="device")):
        b = D.PatchHDRDataset(d, names, True, **kw)
        assert a.shapes == b.shapes and torch.equal(a.arena.view(torch.int32), b.arena.view(torch.int32))
        assert torch.equal(a.means.view(torch.int32), b.means.view(torch.int32))


def test_hdr_real_folder_arena_is_the_same(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(45)
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "HDR_gt"))
    os.makedirs(os.path.join(root, "LDR_in"))
    for i, (comp, t, (h, w)) in enumerate((("piz", X.HALF, (33, 47)), (X.ZIPS, X.FLOAT, (40, 52)), ("piz", X.FLOAT, (70, 32)), (X.RLE, X.HALF, (32, 32)))):
        path = os.path.join(root, "HDR_gt", "s%d.exr" % i)
        if comp == "piz":
            piz_ref.write_exr(path, _channels(h, w, t))
        else:
            X.write_exr(path, _channels(h, w, t), comp)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, "LDR_in", "s%d.jpg" % i), quality=92)
    with pytest.raises(ValueError, match="PIZ compression is not supported"):
        HR.HdrRealFolder(root, size=16, stride=8)
    a = HR.HdrRealFolder(root, size=16, stride=8, exr_piz="host")
    b = HR.HdrRealFolder(root, size=16, stride=8, exr_piz="device")
    assert a.files == b.files and a.shapes == b.shapes
    assert torch.equal(a.hdr_arena.view(torch.int32), b.hdr_arena.view(torch.int32)) and torch.equal(a.ldr_arena, b.ldr_arena)
    assert a.patches == b.patches and np.array_equal(a.means.view(np.uint32), b.means.view(np.uint32))
