"""The device Huffman-only zlib encoder (csrc/deflate.hip, K.deflate_huffman) against the host routine: byte equality, since both run
the code of csrc/deflate_huffman.h.  The host routine itself is judged by zlib in tests/test_deflate_host.py."""
import zlib

import numpy as np
import pytest
import torch

from test_deflate_host import CHUNKS

pytestmark = pytest.mark.gpu


def batch(chunks):
    data = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
    return torch.from_numpy(data).cuda(), offsets


def check(K, chunks, **kw):
    """every chunk's stored bytes: the host stream where it is strictly smaller than the chunk (flag 1), else the chunk (flag 0)"""
    data, offsets = batch(chunks)
    pad, front = kw.get("pad", 0), kw.get("front", 0)
    out, out_offsets, coded = K.deflate_huffman(data, offsets, **kw)
    out, off, coded = out.cpu().numpy(), out_offsets.cpu().numpy(), coded.cpu().numpy()
    assert off[0] == 0 and off.shape == (len(chunks) + 1,) and coded.shape == (len(chunks),)
    for c, chunk in enumerate(chunks):
        host = K.deflate_huffman_host(chunk)
        want_coded = len(host) < len(chunk)
        got = out[front + off[c] + pad:front + off[c + 1]].tobytes()
        assert coded[c] == want_coded, (c, len(chunk))
        assert got == (host if want_coded else chunk), (c, len(chunk))
        if want_coded:
            assert zlib.decompress(got) == chunk
    return coded


def test_mixed_batch_equals_the_host_routine(shdr):
    K = shdr._ops
    rng = np.random.default_rng(21)
    T = K.DEFLATE_TILE
    chunks = [CHUNKS[k] for k in sorted(CHUNKS)]
    chunks.append(rng.integers(0, 256, 50000, dtype=np.uint8).tobytes())                    # white noise: not coded
    for n in (T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 5 * T + 77):                 # the writer's tiles count n + 1 symbols
        chunks.append((128 + rng.integers(-2, 3, n)).astype(np.uint8).tobytes())              # 5 values: coded from ~300 bytes on
        chunks.append((rng.integers(0, 256, n) & 0x33).astype(np.uint8).tobytes())
    ramp = (np.arange(40000) // 157 + rng.integers(0, 3, 40000)).astype(np.uint8).tobytes()
    chunks.append(ramp)
    coded = check(K, chunks)
    assert coded.any() and not coded.all()


def test_thousand_small_chunks(shdr):
    """the scan over more chunks than one round of its block, and the offsets: chunks this small are never coded"""
    rng = np.random.default_rng(22)
    sizes = rng.integers(1, 65, 1000)
    chunks = [rng.integers(0, 4, n, dtype=np.uint8).tobytes() for n in sizes]
    chunks += [bytes([c % 7]) * 3000 for c in range(1100)]                                    # and 1100 coded ones among them
    order = rng.permutation(len(chunks))
    coded = check(shdr._ops, [chunks[i] for i in order])
    assert coded.sum() == 1100


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_offsets_where_the_scan_loops(shdr, n, pad):
    """the one-block scan of the stored sizes (scan_array of csrc/batch.h, 1024 chunks a step; PIZ encode runs the same) on batches
    that end inside, at and one past a step: out_offsets against the host routine's sizes summed here, and every stored chunk"""
    K = shdr._ops
    rng = np.random.default_rng(25)
    chunks = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in rng.integers(1, 4, n)]
    host = {c: K.deflate_huffman_host(c) for c in set(chunks)}
    stored = [host[c] if len(host[c]) < len(c) else c for c in chunks]
    data, offsets = batch(chunks)
    out, out_offsets, coded = K.deflate_huffman(data, offsets, pad=pad)
    out, off, coded = out.cpu().numpy(), out_offsets.cpu().numpy(), coded.cpu().numpy()
    assert off.tolist() == np.concatenate([[0], np.cumsum([pad + len(s) for s in stored])]).tolist()
    assert coded.tolist() == [int(len(host[c]) < len(c)) for c in chunks]
    for c, s in enumerate(stored):
        assert out[off[c] + pad:off[c + 1]].tobytes() == s, c


def test_pad_front_and_raw(shdr):
    """room in front of every chunk and of the whole output stays untouched; a chunk that is not coded is stored from `raw`"""
    K = shdr._ops
    rng = np.random.default_rng(23)
    chunks = [bytes([9]) * 5000, rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), (rng.integers(0, 3, 2049)).astype(np.uint8).tobytes()]
    check(K, chunks, pad=8, front=24)
    data, offsets = batch(chunks)
    raw = torch.flip(data, dims=[0]).contiguous()
    out, out_offsets, coded = K.deflate_huffman(data, offsets, raw=raw, pad=8)
    out, off = out.cpu().numpy(), out_offsets.cpu().numpy()
    assert coded.cpu().tolist() == [1, 0, 1]
    assert out[off[1] + 8:off[2]].tobytes() == raw.cpu().numpy()[offsets[1]:offsets[2]].tobytes()
    assert zlib.decompress(out[off[2] + 8:off[3]].tobytes()) == chunks[2]


def test_one_byte_tile_and_tile_minus_one_with_every_option(shdr):
    """the smallest chunk (stored from `raw`), a chunk of exactly one tile (end-of-block alone in a second tile) and one of a tile
    less one (one tile with it), with pad, front, a buffer of its own for `raw`, host offsets beside their device copy, and stage times"""
    K = shdr._ops
    T = K.DEFLATE_TILE
    rng = np.random.default_rng(24)
    chunks = [b"\x5a", (128 + rng.integers(-2, 3, T)).astype(np.uint8).tobytes(), b"\x07" * (T - 1)]
    data, offsets = batch(chunks)
    kw = dict(raw=data.clone(), pad=8, front=24, offsets_dev=torch.from_numpy(offsets).cuda())
    ms = []
    coded = check(K, chunks, stage_ms=ms, **kw)
    assert coded.tolist() == [0, 1, 1]
    assert len(ms) == 3 and all(v >= 0 for v in ms)
    kw["raw"] = 255 - data                                                    # what is not coded comes from `raw`, not from `data`
    ms = []
    a, b = K.deflate_huffman(data, offsets, stage_ms=ms, **kw), K.deflate_huffman(data, offsets, **kw)
    assert len(ms) == 3 and all(v >= 0 for v in ms)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[2].cpu().tolist() == [0, 1, 1]
    off = a[1].cpu().numpy()
    for c in range(3):                                                        # (the room of pad and front is never written)
        assert torch.equal(a[0][24 + off[c] + 8:24 + off[c + 1]], b[0][24 + off[c] + 8:24 + off[c + 1]]), c
    assert a[0][24 + 8:24 + off[1]].cpu().tolist() == [255 - 0x5a]


def test_same_input_same_bytes_and_stage_times(shdr):
    K = shdr._ops
    data, offsets = batch([CHUNKS["noisy_ramp"], CHUNKS["fibonacci"]])
    a = K.deflate_huffman(data, offsets)
    ms = []
    b = K.deflate_huffman(data, torch.from_numpy(offsets).cuda(), stage_ms=ms)
    total = int(a[1][-1])                                                     # (the buffer is sized by the bound; the rest is not written)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0][:total], b[0][:total])
    assert len(ms) == 3 and all(v >= 0 for v in ms)


def test_refusals(shdr):
    K = shdr._ops
    data = torch.zeros(100, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match="chunk 1 has 0 bytes"):
        K.deflate_huffman(data, np.array([0, 50, 50, 100]))
    with pytest.raises(RuntimeError, match=r"offsets\[0\]"):
        K.deflate_huffman(data, np.array([10, 100]))
    with pytest.raises(ValueError, match="end within"):
        K.deflate_huffman(data, np.array([0, 101]))
    with pytest.raises(RuntimeError, match="pad"):
        K.deflate_huffman(data, np.array([0, 100]), pad=-1)
    with pytest.raises(TypeError):
        K.deflate_huffman(data.float(), np.array([0, 100]))
