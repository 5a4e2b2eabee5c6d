"""The device reader of Radiance scanlines (csrc/hdr_rle_dec.hip, K.rgbe_rle_decode) against its exact oracle, the host twin
shdr_rgbe_rle_decode_status (which tests/test_hdr_rle_dec_host.py holds to the host routine and to an independent NumPy reader), on
every stream of tests/hdr_rle_dec_cases.py: status, failing scanline, consumed / stop offset and the pixels of accepted files, byte
for byte, never a tolerance.  Every stream goes through the decoder alone-in-its-class (one call per batch of a few hundred files of
mixed shapes, and batches of one), with guard bytes around the output and known bytes in every slot, so that what a refused or
FALLBACK file leaves alone is seen.  The shapes are the cases': widths around every boundary of the format, 65 rows (more than a wave
has lanes), the widest coded line, files cut at every length."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import hdr_rle_dec_cases as C
import hdr_rle_dec_ref as REF
import hdr_rle_ref as R

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
IO, K, LIB = pkg.hdr_io, pkg._ops, pkg._lib

GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def twin():
    """name -> (pixels or None, status, line, consumed) of the host twin; FALLBACK where the device hands the file back"""
    out = {}
    for name, w, h, data in C.cases():
        if REF.count_candidates(data, w) > 2 * h + 64:
            out[name] = (None, K.RGBE_DEC_FALLBACK, -1, -1)
        else:
            out[name] = K.rgbe_rle_decode_host(data, w, h)
    return out


def _decode(batch):
    """the C ABI on a batch of (name, w, h, data) with a guarded, pre-filled output: (out with guards [host], out_off, status, line,
    consumed) as host arrays"""
    lib = LIB.load()
    n = len(batch)
    shapes = np.array([(h, w) for _, w, h, _ in batch], dtype=np.int32)
    src_off = np.concatenate([[0], np.cumsum([len(d) for _, _, _, d in batch])]).astype(np.int64)
    blob = np.frombuffer(b"".join(d for _, _, _, d in batch) + b"\0", dtype=np.uint8)
    out_b, ws_b = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.shdr_rgbe_rle_decode_batch_sizes(shapes.ctypes.data, src_off.ctypes.data, n, ctypes.byref(out_b), ctypes.byref(ws_b)) == 0
    assert out_b.value == int(4 * (shapes[:, 0].astype(np.int64) * shapes[:, 1]).sum())
    src = torch.from_numpy(blob.copy()).cuda()
    out = torch.full((out_b.value + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.full((ws_b.value + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    line = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    consumed = torch.full((n,), -9, dtype=torch.int64, device="cuda")
    s_dev, shapes_dev = torch.from_numpy(src_off).cuda(), torch.from_numpy(shapes).cuda()
    rc = lib.shdr_rgbe_rle_decode_batch(src.data_ptr(), int(src_off[-1]), src_off.ctypes.data, s_dev.data_ptr(), shapes.ctypes.data,
                                        shapes_dev.data_ptr(), n, out.data_ptr() + GUARD, out_b.value, out_off.data_ptr(),
                                        ws.data_ptr() + GUARD, ws_b.value, status.data_ptr(), line.data_ptr(), consumed.data_ptr(),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None)
    assert rc == 0, lib.shdr_last_error()
    torch.cuda.synchronize()
    ws_host = ws.cpu().numpy()
    assert (ws_host[:GUARD] == 0x5A).all() and (ws_host[-GUARD:] == 0x5A).all()           # _batch_sizes against the buffer used
    return out.cpu().numpy(), out_off.cpu().numpy(), status.cpu().numpy(), line.cpu().numpy(), consumed.cpu().numpy()


def _check(batch, twin):
    out, out_off, status, line, consumed = _decode(batch)
    assert (out[:GUARD] == FILL).all() and (out[-GUARD:] == FILL).all(), "guard bytes around the output"
    body = out[GUARD:-GUARD]
    want_off = np.concatenate([[0], np.cumsum([4 * w * h for _, w, h, _ in batch])])
    assert np.array_equal(out_off, want_off)
    for i, (name, w, h, data) in enumerate(batch):
        pixels, st, ln, cons = twin[name]
        assert (int(status[i]), int(line[i]), int(consumed[i])) == (st, ln, cons), (name, i, (status[i], line[i], consumed[i]), (st, ln, cons))
        slot = body[want_off[i]:want_off[i + 1]]
        if st == K.RGBE_DEC_OK:
            if not np.array_equal(slot, pixels.reshape(-1)):
                at = int(np.flatnonzero(slot != pixels.reshape(-1))[0])
                raise AssertionError("%s (file %d, %d x %d): first difference at byte %d (row %d, pixel %d, component %d): %d != %d" % (
                    name, i, h, w, at, at // (4 * w), at % (4 * w) // 4, at % 4, slot[at], pixels.reshape(-1)[at]))
        elif st == K.RGBE_DEC_FALLBACK:
            assert (slot == FILL).all(), "%s: a FALLBACK file's slot is not written" % name


def _batches(size):
    """the cases in batches of about `size` files, the large files spread out, neighbours of different shapes"""
    cases = sorted(C.cases(), key=lambda c: len(c[3]))
    k = max(1, -(-len(cases) // size))
    return [cases[i::k] for i in range(k)]


def test_every_case_in_batches_of_several_hundred(twin):
    for batch in _batches(400):
        assert len(batch) >= 300
        _check(batch, twin)


def test_every_case_in_small_mixed_batches(twin):
    # refused and FALLBACK files between accepted ones: the slots left and right of them are exact
    named = C.by_name()
    good = [named[n] for n in ("families_9x3", "families_257x2", "families_7x3", "one_byte_literals", "literal_128")]
    bad = [c for c in C.cases() if twin[c[0]][1] != 0 and not c[0].startswith(("prefix_", "byte_"))]
    bad += [c for c in C.cases() if c[0].startswith("prefix_")][::9] + [c for c in C.cases() if c[0].startswith("byte_")][::31]
    assert {twin[c[0]][1] for c in bad} >= {1, 2, 3, 4, 5}                              # (some mutated files are still accepted)
    batch = []
    for i, c in enumerate(bad):
        batch += [good[i % len(good)], c]
    batch.append(good[0])
    _check(batch, twin)
    _check(batch[::-1], twin)


def test_batches_of_one(twin):
    names = ["families_8x1", "families_1x65", "families_514x65", "families_32767_1", "flat_32768", "dense_514", "dense_514_flat", "dense_514_then_coded", "size_0", "markers_at_cap_h3",
             "markers_over_cap_h1", "run_overshoots_by_one", "flat_line_one_byte_short", "zero_counts_longer_than_a_window",
             "flat_with_whole_line_at_4", "markers_at_cap_in_flat_lines", "prefix_mixed_40"]
    named = C.by_name()
    for name in names:
        _check([named[name]], twin)


def test_the_same_input_gives_the_same_bytes(twin):
    batch = _batches(400)[0][:200]
    a, b = _decode(batch), _decode(batch)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_ops_wrapper_and_stage_times(twin):
    named = C.by_name()
    batch = [named[n] for n in ("families_129x65", "dense_514", "prefix_coded_30", "families_7x2")]
    shapes = [(h, w) for _, w, h, _ in batch]
    src_off = np.concatenate([[0], np.cumsum([len(c[3]) for c in batch])])
    src = torch.from_numpy(np.frombuffer(b"".join(c[3] for c in batch), dtype=np.uint8).copy()).cuda()
    ms = []
    out, out_off, status, line, consumed = K.rgbe_rle_decode(src, src_off, shapes, stage_ms=ms)
    assert len(ms) == 4 and all(t >= 0 for t in ms)
    assert status.tolist() == [twin[c[0]][1] for c in batch] and line.tolist() == [twin[c[0]][2] for c in batch]
    assert consumed.tolist() == [twin[c[0]][3] for c in batch]
    off = out_off.tolist()
    for i in (0, 3):
        assert np.array_equal(out[off[i]:off[i + 1]].cpu().numpy(), twin[batch[i][0]][0].reshape(-1))
    with pytest.raises(TypeError):
        K.rgbe_rle_decode(src.cpu(), src_off, shapes)
    with pytest.raises(ValueError):
        K.rgbe_rle_decode(src, src_off[:-1], shapes)


# --- through hdr_io -------------------------------------------------------------------------------------------------------------------
def _lines(name):
    _, w, h, data = C.by_name()[name]
    return IO.Scanlines(h, w, data, path=name + ".hdr")


def test_rle_decode_device_falls_back_on_the_dense_case():
    items = [_lines("families_9x3"), _lines("dense_514_flat"), _lines("dense_514_then_coded"), _lines("families_257x2")]
    got = IO.rle_decode_device(items)
    assert len(got) == 4
    for it, t in zip(items, got):
        assert t.is_cuda and t.dtype == torch.uint8 and tuple(t.shape) == it.shape
        assert np.array_equal(t.cpu().numpy(), IO.rle_decode(it.data, it.height, it.width))
    with pytest.raises(ValueError) as exc:                                  # a FALLBACK file that the host routine refuses
        IO.rle_decode_device(items + [_lines("dense_514")])
    assert str(exc.value) == "dense_514.hdr: rgbe_rle_decode: truncated data in scanline 2"


def test_first_bad_file_raises_the_host_message():
    items = [_lines("families_9x3"), _lines("literal_overshoots_by_one"), _lines("run_overshoots_by_one")]
    with pytest.raises(ValueError) as exc:
        IO.rle_decode_device(items)
    with pytest.raises(ValueError) as host:
        IO.rle_decode(items[1].data, items[1].height, items[1].width)
    assert str(exc.value) == "literal_overshoots_by_one.hdr: %s" % host.value == "literal_overshoots_by_one.hdr: rgbe_rle_decode: corrupt literal in scanline 0"
    with pytest.raises(ValueError) as exc:
        IO.rle_decode_device([items[0], IO.Scanlines(2, 16, items[2].data)])
    assert str(exc.value) == "scanlines[1]: rgbe_rle_decode: corrupt run in scanline 1"


def test_read_rgbe_on_the_device_equals_the_host(tmp_path):
    paths = []
    for i, (h, w) in enumerate(((5, 9), (3, 7), (2, 300), (67, 128))):
        path = str(tmp_path / ("f%d.hdr" % i))
        IO.write_hdr(path, R.family_image(h, w, seed=20 + i))
        paths.append(path)
    for path in paths:
        dev = IO.read_rgbe(path, decoder="device")
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), IO.read_rgbe(path))
    for a, b in zip(IO.read_rgbe_batch(paths, decoder="device"), IO.read_rgbe_batch(paths)):
        assert np.array_equal(a.cpu().numpy(), b)
    with open(paths[0], "rb") as f:
        data = f.read()
    with open(paths[0], "wb") as f:
        f.write(data[:-3])
    with pytest.raises(ValueError) as exc:
        IO.read_rgbe_batch(paths[::-1], decoder="device")
    with pytest.raises(ValueError) as host:
        IO.read_rgbe(paths[0])
    assert str(exc.value) == str(host.value) and paths[0] in str(exc.value)


def test_round_trip_of_a_noisy_ramp_batch_on_the_device():
    g = torch.Generator(device="cuda").manual_seed(1)
    images = []
    for h, w in ((67, 301), (5, 1000), (130, 64)):
        yy, xx = torch.meshgrid(torch.linspace(0, 1, h, device="cuda"), torch.linspace(0, 1, w, device="cuda"), indexing="ij")
        ramp = torch.stack((4.0 * xx, 0.5 * yy + 0.1, xx * yy), dim=-1)
        images.append(K.rgbe_encode((ramp * (1 + 0.02 * torch.randn(ramp.shape, device="cuda", generator=g))).contiguous()))
    data, offsets = K.rgbe_rle_encode(images)                                   # the coded bytes stay on the device ...
    off = offsets.cpu().numpy()
    out, out_off, status, line, consumed = K.rgbe_rle_decode(data[:int(off[-1])], off, [t.shape[:2] for t in images])       # ... the offsets are a host table
    assert status.tolist() == [0, 0, 0] and consumed.tolist() == np.diff(off).tolist()
    o = out_off.tolist()
    for i, t in enumerate(images):
        assert torch.equal(out[o[i]:o[i + 1]].view(t.shape), t)
    got = IO.rle_decode_device([IO.Scanlines(t.shape[0], t.shape[1], d) for t, d in zip(images, IO.rle_encode_device(images))])
    assert all(torch.equal(a, b) for a, b in zip(got, images))


# --- the C ABI with ctypes alone --------------------------------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments():
    lib = LIB.load()
    _, w, h, data = C.by_name()["families_9x3"]
    shapes = np.array([(h, w), (h, w)], dtype=np.int32)
    src_off = np.array([0, len(data), 2 * len(data)], dtype=np.int64)
    out_b, ws_b = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.shdr_rgbe_rle_decode_batch_sizes(shapes.ctypes.data, src_off.ctypes.data, 2, ctypes.byref(out_b), ctypes.byref(ws_b)) == 0
    assert out_b.value == 2 * 4 * w * h and ws_b.value > 0 and ws_b.value % 16 == 0
    src = torch.from_numpy(np.frombuffer(data * 2, dtype=np.uint8).copy()).cuda()
    out = torch.full((out_b.value + 16,), FILL, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(ws_b.value + 16, dtype=torch.uint8, device="cuda")
    out_off = torch.zeros(3, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -9, dtype=torch.int32, device="cuda")
    line, consumed = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    s_dev, shapes_dev = torch.from_numpy(src_off).cuda(), torch.from_numpy(shapes).cuda()

    def call(**kw):
        a = dict(src=src.data_ptr(), src_bytes=src.numel(), src_off=src_off.ctypes.data, src_off_dev=s_dev.data_ptr(),
                 shapes=shapes.ctypes.data, shapes_dev=shapes_dev.data_ptr(), n=2, out=out.data_ptr(), out_bytes=out_b.value,
                 out_off=out_off.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws_b.value, status=status.data_ptr(), line=line.data_ptr(),
                 consumed=consumed.data_ptr())
        a.update(kw)
        return lib.shdr_rgbe_rle_decode_batch(a["src"], a["src_bytes"], a["src_off"], a["src_off_dev"], a["shapes"], a["shapes_dev"], a["n"],
                                              a["out"], a["out_bytes"], a["out_off"], a["ws"], a["ws_bytes"], a["status"], a["line"],
                                              a["consumed"], None, None)

    for name in ("src", "src_off", "src_off_dev", "shapes", "shapes_dev", "out", "out_off", "ws", "status", "line", "consumed"):
        assert call(**{name: None}) != 0, name
        assert b"rgbe_rle_decode_batch" in lib.shdr_last_error()
    assert call(ws=ws.data_ptr() + 8) != 0 and b"aligned" in lib.shdr_last_error()                  # a misaligned workspace
    assert call(out=out.data_ptr() + 2) != 0 and b"aligned" in lib.shdr_last_error()
    assert call(ws_bytes=ws_b.value - 1) != 0 and b"workspace" in lib.shdr_last_error()             # one byte short
    assert call(out_bytes=out_b.value - 1) != 0
    assert call(src_bytes=src.numel() - 1) != 0
    assert call(n=0) != 0
    bad_off = np.array([0, 2 * len(data), len(data)], dtype=np.int64)                              # offsets out of order
    assert call(src_off=bad_off.ctypes.data) != 0 and b"decreases" in lib.shdr_last_error()
    assert lib.shdr_rgbe_rle_decode_batch_sizes(shapes.ctypes.data, bad_off.ctypes.data, 2, ctypes.byref(out_b), ctypes.byref(ws_b)) != 0
    bad_shapes = np.array([(h, w), (0, w)], dtype=np.int32)
    assert call(shapes=bad_shapes.ctypes.data) != 0
    assert lib.shdr_rgbe_rle_decode_batch_sizes(None, src_off.ctypes.data, 2, ctypes.byref(out_b), ctypes.byref(ws_b)) != 0
    torch.cuda.synchronize()
    assert status.tolist() == [-9, -9] and (out.cpu().numpy() == FILL).all()                       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and consumed.tolist() == [len(data)] * 2
    want = IO.rle_decode(data, h, w).reshape(-1)
    got = out.cpu().numpy()
    assert np.array_equal(got[:out_b.value], np.concatenate([want, want])) and (got[out_b.value:] == FILL).all()
