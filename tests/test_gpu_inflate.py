"""The device inflate (csrc/inflate.hip, K.inflate) on the lists of tests/test_inflate_host.py: byte equality with zlib for the streams the
oracle accepts, a non-zero status exactly where it refuses, and in every case the status, the byte count and the bytes of the host twin
(both run csrc/inflate.h).  Slots are surrounded by guard bytes, sources and slots lie at every byte alignment."""
import zlib

import numpy as np
import pytest
import torch

import deflate_synth as S
from test_deflate_host import CHUNKS
from test_inflate_host import INVALID, VALID, ZLIB

pytestmark = pytest.mark.gpu

FILL = 0xC3
RAW_SIZE = 19            # SHDR_INFLATE_RAW_SIZE


def run_batch(K, items, src_align=None, lead=1):
    """items: [(bytes, want, mode)].  In front of every chunk lies a GUARD chunk: mode 0 (stored raw) with a source of g bytes and a slot of
    h != g bytes, which the kernel must refuse and leave alone; g puts the chunk's source at byte alignment src_align[c % len] (relative to
    the 256-byte aligned buffer), h = 1 or 3 keeps the slots at changing, mostly odd offsets.  The first slot starts at `lead`.  Checks
    everything against the oracle and the host twin; returns (status, written) of the real chunks."""
    src, s_off, d_off, modes = bytearray(), [0], [lead], []
    for c, (data, want, mode) in enumerate(items):
        g = 2
        if src_align is not None:
            g = (src_align[c % len(src_align)] - len(src)) % 8
            g += 8 if g == 3 else 0
        h = 3 if g != 3 else 1
        src += bytes([0x5A]) * g
        s_off.append(len(src))
        d_off.append(d_off[-1] + h)
        modes.append(0)
        src += data
        s_off.append(len(src))
        d_off.append(d_off[-1] + want)
        modes.append(mode)
    dst = torch.full((d_off[-1] + 7,), FILL, dtype=torch.uint8, device="cuda")
    out, written, status = K.inflate(torch.frombuffer(bytearray(src) or bytearray(1), dtype=torch.uint8).cuda()[:len(src)], np.array(s_off),
                                     np.array(d_off), mode=torch.tensor(modes, dtype=torch.uint8, device="cuda"), dst=dst)
    assert out.data_ptr() == dst.data_ptr()
    out, written, status = out.cpu().numpy(), written.cpu().numpy(), status.cpu().numpy()
    assert np.all(out[:lead] == FILL) and np.all(out[d_off[-1]:] == FILL)
    for c, (data, want, mode) in enumerate(items):
        g, r = 2 * c, 2 * c + 1
        assert status[g] == RAW_SIZE and written[g] == 0 and np.all(out[d_off[g]:d_off[g + 1]] == FILL), "guard %d" % c
        slot = out[d_off[r]:d_off[r + 1]]
        assert 0 <= written[r] <= want
        assert np.all(slot[written[r]:] == FILL), "chunk %d: bytes beyond `written` were touched" % c
        if mode == 0:
            if len(data) == want:
                assert status[r] == 0 and written[r] == want and slot.tobytes() == data
            else:
                assert status[r] == RAW_SIZE and written[r] == 0
            continue
        host_bytes, host_status = K.inflate_host(data, want)
        assert (status[r], written[r]) == (host_status, len(host_bytes)), "chunk %d: device %d / %d, host %d / %d" % (
            c, status[r], written[r], host_status, len(host_bytes))
        assert slot[:written[r]].tobytes() == host_bytes
        if S.accepts(data, want):
            assert status[r] == 0 and slot.tobytes() == zlib.decompress(data)
        else:
            assert status[r] != 0
    return status[1::2], written[1::2]


def test_one_chunk(shdr):
    name, stream, want = VALID[0]
    status, written = run_batch(shdr._ops, [(stream, want, 1)])
    assert status.tolist() == [0] and written.tolist() == [want]


def test_two_chunks(shdr):
    by_name = {n: (s, w, 1) for n, s, w in VALID}
    status, _ = run_batch(shdr._ops, [by_name["overlaps_dynamic"], by_name["match_across_blocks_and_types"]])
    assert status.tolist() == [0, 0]


def test_synthetic_valid_streams(shdr):
    status, written = run_batch(shdr._ops, [(s, w, 1) for _, s, w in VALID])
    assert not status.any() and written.tolist() == [w for _, _, w in VALID]


def test_synthetic_invalid_streams(shdr):
    """only these hand-listed classes of malformed bytes go to the device; the exhaustive sweep runs on the host"""
    status, _ = run_batch(shdr._ops, [(s, w, 1) for _, s, w in INVALID])
    assert status.all()


def test_300_chunks_of_mixed_sizes_in_one_launch(shdr):
    small = [(s, w, 1) for _, s, w in VALID + INVALID if w < 4000]
    items = ([(s, w, 1) for _, s, w in ZLIB if w < 10000] + small)
    items = (items + small * 3)[:300]
    assert len(items) == 300
    status, _ = run_batch(shdr._ops, items)
    assert (status == 0).sum() > 200 and (status != 0).sum() > 40


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_sources_at_all_eight_alignments(shdr, lead):
    pick = [c for c in VALID if c[0] in ("every_length_dynamic", "overlaps_fixed", "stored_after_unaligned_dynamic", "output_1", "output_0_stored",
                                         "match_across_blocks_and_types", "code_of_15_bits", "several_dynamic_blocks")]
    assert len(pick) == 8
    for shift in range(8):
        order = [(k + shift) % 8 for k in range(8)]                   # every stream meets every alignment
        run_batch(shdr._ops, [(s, w, 1) for _, s, w in pick], src_align=order, lead=lead)


def test_zlib_level_0_of_70000_bytes(shdr):
    item = [(s, w, 1) for n, s, w in ZLIB if n == "random_70000_l0"]
    status, _ = run_batch(shdr._ops, item, src_align=[5])
    assert status.tolist() == [0]


def test_raw_chunks_mixed_in(shdr):
    rng = np.random.default_rng(3)
    raw = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1, 7, 64, 1000, 4097)]
    by_name = {n: (s, w, 1) for n, s, w in VALID}
    items = [(raw[0], 1, 0), by_name["overlaps_fixed"], (raw[1], 7, 0), (raw[2], 65, 0), by_name["output_1"], (raw[3], 1000, 0),
             (raw[4], 4096, 0), (b"", 0, 0), by_name["hdist_0_zero_length"], (raw[4], 4097, 0)]
    status, written = run_batch(shdr._ops, items)
    assert status.tolist() == [0, 0, 0, RAW_SIZE, 0, 0, RAW_SIZE, 0, 0, 0]


def test_empty_streams(shdr):
    empty = zlib.compress(b"")
    status, written = run_batch(shdr._ops, [(b"", 0, 1), (empty, 0, 1), (b"", 5, 1), (empty, 1, 1)])
    assert status.tolist() == [1, 0, 1, 17] and written.tolist() == [0, 0, 0, 0]


def test_mode_bytes_other_than_0_and_1_are_refused(shdr):
    K = shdr._ops
    stream = zlib.compress(b"abc")
    src = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    dst, written, status = K.inflate(src, np.array([0, len(stream)]), np.array([0, 3]), mode=torch.tensor([2], dtype=torch.uint8, device="cuda"))
    assert status.tolist() == [20] and written.tolist() == [0]
    dst, written, status = K.inflate(src, np.array([0, len(stream)]), np.array([0, 3]))          # default: all zlib
    assert status.tolist() == [0] and bytes(dst.cpu().numpy()) == b"abc"


def test_the_device_encoders_output_comes_back(shdr):
    K = shdr._ops
    names = ["len1", "len257", "one_byte_repeated", "all_256_values", "noisy_ramp", "ff_70000"]
    data = b"".join(CHUNKS[n] for n in names)
    offsets = np.cumsum([0] + [len(CHUNKS[n]) for n in names]).astype(np.int64)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out, out_offsets, coded = K.deflate_huffman(dev, offsets)
    back, written, status = K.inflate(out, out_offsets, offsets, mode=coded)                    # coded == 0: stored raw
    assert not status.cpu().any() and written.cpu().tolist() == np.diff(offsets).tolist()
    assert torch.equal(back, dev)
    assert coded.cpu().tolist().count(1) >= 3


def test_deterministic_and_timed(shdr):
    K = shdr._ops
    streams = [s for _, s, _ in ZLIB[:40]]
    wants = [w for _, _, w in ZLIB[:40]]
    src = torch.frombuffer(bytearray(b"".join(streams)), dtype=torch.uint8).cuda()
    s_off, d_off = np.cumsum([0] + [len(s) for s in streams]), np.cumsum([0] + wants)
    a = K.inflate(src, s_off, d_off)
    ms = []
    b = K.inflate(src, torch.from_numpy(s_off).cuda(), torch.from_numpy(d_off).cuda(), stage_ms=ms)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert len(ms) == 1 and ms[0] > 0
    assert bytes(a[0].cpu().numpy()) == b"".join(zlib.decompress(s) for s in streams)


def test_refusals(shdr):
    K = shdr._ops
    src = torch.zeros(100, dtype=torch.uint8, device="cuda")
    ok = np.array([0, 50, 100])
    with pytest.raises(RuntimeError, match="chunk 1 has -10 bytes in src_off"):
        K.inflate(src, np.array([0, 60, 50]), ok)
    with pytest.raises(RuntimeError, match="chunk 0 has -1 bytes in dst_off"):
        K.inflate(src, ok, np.array([1, 0, 5]))
    with pytest.raises(RuntimeError, match=r"src_off\[0\] is negative"):
        K.inflate(src, np.array([-1, 50, 100]), ok)
    with pytest.raises(ValueError, match="src holds 100 bytes"):
        K.inflate(src, np.array([0, 50, 101]), ok)
    with pytest.raises(ValueError, match="two offset tables"):
        K.inflate(src, ok, np.array([0, 50]))
    with pytest.raises(ValueError, match="dst holds 10 bytes"):
        K.inflate(src, ok, ok, dst=torch.zeros(10, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="mode must be"):
        K.inflate(src, ok, ok, mode=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="2\\^30"):
        K.inflate(src, ok, np.array([0, 50, 50 + (1 << 30) + 1]), dst=torch.zeros(10, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        K.inflate(src.float(), ok, ok)
