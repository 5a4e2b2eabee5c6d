"""The device LZ77 zlib encoder (csrc/deflate_lz.hip, K.deflate_lz) against the host routine: byte equality, since both run the code of
csrc/deflate_lz.h.  The host routine itself is judged by zlib in tests/test_deflate_lz_host.py."""
import zlib

import numpy as np
import pytest
import torch

from deflate_lz_cases import CASES

pytestmark = pytest.mark.gpu


def batch(chunks):
    data = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
    return torch.from_numpy(data).cuda(), offsets


def check(K, chunks, **kw):
    """every chunk's stored bytes: the host stream where it is strictly smaller than the chunk (flag 1), else the chunk (flag 0);
    then the device decoder on the stored batch"""
    data, offsets = batch(chunks)
    pad, front = kw.get("pad", 0), kw.get("front", 0)
    out_dev, out_offsets, coded_dev = K.deflate_lz(data, offsets, **kw)
    out, off, coded = out_dev.cpu().numpy(), out_offsets.cpu().numpy(), coded_dev.cpu().numpy()
    assert off[0] == 0 and off.shape == (len(chunks) + 1,) and coded.shape == (len(chunks),)
    host = {}
    for c, chunk in enumerate(chunks):
        if chunk not in host:
            host[chunk] = K.deflate_lz_host(chunk)
            assert zlib.decompress(host[chunk]) == chunk
        want_coded = len(host[chunk]) < len(chunk)
        got = out[front + off[c] + pad:front + off[c + 1]].tobytes()
        assert coded[c] == want_coded, (c, len(chunk))
        assert got == (host[chunk] if want_coded else chunk), (c, len(chunk))
    if pad == 0:
        back, written, status = K.inflate(out_dev[front:], out_offsets, offsets, mode=coded_dev)
        assert status.cpu().tolist() == [0] * len(chunks) and written.cpu().tolist() == [len(c) for c in chunks]
        assert torch.equal(back[:data.numel()], data)
    return coded


def test_aimed_cases_equal_the_host_routine(shdr):
    K = shdr._ops
    rng = np.random.default_rng(41)
    T = K.DEFLATE_LZ_TILE
    chunks = [CASES[k] for k in sorted(CASES)]
    for n in (T - 1, T, T + 1, 2 * T + 1):                                                   # the writer's tiles count n + 1 positions
        chunks.append((128 + rng.integers(-2, 3, n)).astype(np.uint8).tobytes())              # short matches and literals
        chunks.append((np.arange(n) // 37 % 5).astype(np.uint8).tobytes())                    # runs that cross the tiles
    coded = check(K, chunks)
    assert coded.any() and not coded.all()


def test_thousand_small_chunks(shdr):
    """the scan over more chunks than one round of its block, and the offsets: chunks this small are never coded"""
    rng = np.random.default_rng(42)
    sizes = rng.integers(1, 65, 1000)
    chunks = [rng.integers(0, 4, n, dtype=np.uint8).tobytes() for n in sizes]
    chunks += [bytes([c % 7]) * 1500 + bytes(range(c % 7, c % 7 + 40)) * 30 for c in range(1100)]   # and 1100 coded ones among them
    order = rng.permutation(len(chunks))
    coded = check(shdr._ops, [chunks[i] for i in order])
    assert coded.sum() == 1100


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_offsets_where_the_scan_loops(shdr, n, pad):
    """the one-block scan of the stored sizes (scan_array of csrc/batch.h, 1024 chunks a step) on batches that end inside, at and one
    past a step: out_offsets against the host routine's sizes summed here, and every stored chunk"""
    K = shdr._ops
    rng = np.random.default_rng(45)
    chunks = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in rng.integers(1, 4, n)]
    host = {c: K.deflate_lz_host(c) for c in set(chunks)}
    stored = [host[c] if len(host[c]) < len(c) else c for c in chunks]
    data, offsets = batch(chunks)
    out, out_offsets, coded = K.deflate_lz(data, offsets, pad=pad)
    out, off, coded = out.cpu().numpy(), out_offsets.cpu().numpy(), coded.cpu().numpy()
    assert off.tolist() == np.concatenate([[0], np.cumsum([pad + len(s) for s in stored])]).tolist()
    assert coded.tolist() == [int(len(host[c]) < len(c)) for c in chunks]
    for c, s in enumerate(stored):
        assert out[off[c] + pad:off[c + 1]].tobytes() == s, c


def wide_chunk():
    """about 400 KB, the chunk of a 4096-wide HALF ZIP file: 32 rows of 12288 bytes that repeat the row above but for 400 bytes.  A row
    is 256 times an 8-byte word and a 40-byte run, about 2900 different byte triples, so the 4096 slots still hold the row above"""
    rng = np.random.default_rng(43)
    row = np.concatenate([np.concatenate([rng.integers(0, 256, 8), np.full(40, rng.integers(0, 256))]) for _ in range(256)]).astype(np.uint8)
    rows = np.tile(row, (32, 1))
    rows[rng.integers(0, 32, 400), rng.integers(0, 12288, 400)] ^= 0x55
    return rows.tobytes()


def test_a_wide_zip_chunk(shdr):
    chunk = wide_chunk()
    assert len(chunk) == 393216
    coded = check(shdr._ops, [chunk, chunk[:100000]])
    assert coded.tolist() == [1, 1]
    tokens = shdr._ops.deflate_lz_parse_host(chunk)
    assert sum(n for _, n, d in tokens if d == 12288) > len(chunk) // 2               # most of it is the row above


def test_pad_front_and_raw(shdr):
    """room in front of every chunk and of the whole output stays untouched; a chunk that is not coded is stored from `raw`"""
    K = shdr._ops
    rng = np.random.default_rng(44)
    chunks = [bytes([9]) * 5000, rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), (rng.integers(0, 3, 2049)).astype(np.uint8).tobytes()]
    check(K, chunks, pad=8, front=24)
    data, offsets = batch(chunks)
    raw = torch.flip(data, dims=[0]).contiguous()
    got, out_offsets, coded = K.deflate_lz(data, offsets, raw=raw, pad=8)
    got, off = got.cpu().numpy(), out_offsets.cpu().numpy()
    assert coded.cpu().tolist() == [1, 0, 1]
    assert got[off[1] + 8:off[2]].tobytes() == raw.cpu().numpy()[offsets[1]:offsets[2]].tobytes()
    assert zlib.decompress(got[off[2] + 8:off[3]].tobytes()) == chunks[2]


def test_one_byte_tile_and_tile_minus_one_with_every_option(shdr):
    """the smallest chunk (stored from `raw`), a chunk of exactly one tile (end-of-block alone in a second tile) and one of a tile
    less one (one tile with it), with pad, front, a buffer of its own for `raw`, host offsets beside their device copy, and stage times"""
    K = shdr._ops
    T = K.DEFLATE_LZ_TILE
    rng = np.random.default_rng(45)
    chunks = [b"\x5a", (128 + rng.integers(-2, 3, T)).astype(np.uint8).tobytes(), b"\x07" * (T - 1)]
    data, offsets = batch(chunks)
    kw = dict(raw=data.clone(), pad=8, front=24, offsets_dev=torch.from_numpy(offsets).cuda())
    ms = []
    coded = check(K, chunks, stage_ms=ms, **kw)
    assert coded.tolist() == [0, 1, 1]
    assert len(ms) == 3 and all(v >= 0 for v in ms)
    kw["raw"] = 255 - data                                                    # what is not coded comes from `raw`, not from `data`
    ms = []
    a, b = K.deflate_lz(data, offsets, stage_ms=ms, **kw), K.deflate_lz(data, offsets, **kw)
    assert len(ms) == 3 and all(v >= 0 for v in ms)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[2].cpu().tolist() == [0, 1, 1]
    off = a[1].cpu().numpy()
    for c in range(3):                                                        # (the room of pad and front is never written)
        assert torch.equal(a[0][24 + off[c] + 8:24 + off[c + 1]], b[0][24 + off[c] + 8:24 + off[c + 1]]), c
    assert a[0][24 + 8:24 + off[1]].cpu().tolist() == [255 - 0x5a]


def test_same_input_same_bytes_and_stage_times(shdr):
    K = shdr._ops
    data, offsets = batch([CASES["noisy_ramp"], CASES["fibonacci"], CASES["distance_24577"]])
    ms_a, ms_b = [], []
    a = K.deflate_lz(data, offsets, stage_ms=ms_a)
    b = K.deflate_lz(data, torch.from_numpy(offsets).cuda(), stage_ms=ms_b)
    total = int(a[1][-1])                                                     # (the buffer is sized by the bound; the rest is not written)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0][:total], b[0][:total])
    assert len(ms_a) == 3 and len(ms_b) == 3 and all(v >= 0 for v in ms_a + ms_b)


def test_refusals(shdr):
    K = shdr._ops
    data = torch.zeros(100, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match="chunk 1 has 0 bytes"):
        K.deflate_lz(data, np.array([0, 50, 50, 100]))
    with pytest.raises(RuntimeError, match=r"offsets\[0\]"):
        K.deflate_lz(data, np.array([10, 100]))
    with pytest.raises(ValueError, match="end within"):
        K.deflate_lz(data, np.array([0, 101]))
    with pytest.raises(RuntimeError, match="pad"):
        K.deflate_lz(data, np.array([0, 100]), pad=-1)
    with pytest.raises(TypeError):
        K.deflate_lz(data.float(), np.array([0, 100]))
