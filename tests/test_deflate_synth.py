"""The bit-level zlib stream builder (tests/deflate_synth.py) against zlib itself: every stream it calls valid decodes to what its tokens
say, every stream it calls invalid is refused by the rule the EXR reader applies, and the streams hold the features they are named for."""
import zlib

import pytest

import deflate_synth as S

BLOCKS = S._valid_blocks()
VALID = S.valid_cases()
INVALID = S.invalid_cases()


def first_block_type(stream):
    return (stream[2] >> 1) & 3


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_valid_stream_decodes_to_its_tokens(name):
    blocks = BLOCKS[name]
    stream = S.zstream(blocks)
    want = S.expand(blocks)
    d = zlib.decompressobj()
    assert d.decompress(stream) == want and d.eof and d.unused_data == b""
    assert S.accepts(stream, len(want))
    assert not S.accepts(stream, len(want) + 1)
    assert len(want) == 0 or not S.accepts(stream, len(want) - 1)


@pytest.mark.parametrize("name,stream,want", VALID, ids=[c[0] for c in VALID])
def test_valid_case_is_accepted(name, stream, want):
    assert S.accepts(stream, want)


@pytest.mark.parametrize("name,stream,want", INVALID, ids=[c[0] for c in INVALID])
def test_invalid_case_is_refused(name, stream, want):
    assert not S.accepts(stream, want)


def test_names_are_unique():
    names = [c[0] for c in VALID + INVALID]
    assert len(set(names)) == len(names)


def test_distance_32768_after_32768_literals():
    """zlib's compressor never emits it (its window keeps 262 bytes back); its inflate takes it"""
    toks = S.noise(32768, 14) + [("match", 258, 32768)]
    data = zlib.decompress(S.zstream([S.fixed(toks)]))
    assert len(data) == 32768 + 258 and data[32768:] == data[:258]


def test_every_length_and_distance_symbol_is_used():
    lit, _ = S.token_symbols(BLOCKS["every_length_fixed"][0]["tokens"])
    assert {s for s in lit if s > 256} == set(range(257, 286))
    toks = BLOCKS["every_distance_fixed"][0]["tokens"]
    dists = {t[2] for t in toks if t[0] == "match"}
    for s in range(30):
        assert S.DIST_BASE[s] in dists and S.DIST_BASE[s] + (1 << S.DIST_EXTRA[s]) - 1 in dists
    assert 32768 in dists and 1 in dists
    assert {t[1] for t in toks if t[0] == "match"} <= set(range(3, 259))


def test_overlap_cases_are_all_there():
    got = {(t[2], t[1]) for t in BLOCKS["overlaps_fixed"][0]["tokens"] if t[0] == "match"}
    assert got == {(D, L) for D in (1, 2, 3, 63, 64, 65) for L in (3, 63, 64, 65, 128, 129, 258) if D < L}


@pytest.mark.parametrize("name,symbol", [("run_16_crosses_boundary", 16), ("run_17_crosses_boundary", 17), ("run_18_crosses_boundary", 18)])
def test_runs_cross_the_literal_distance_boundary(name, symbol):
    blk = BLOCKS[name][0]
    crossing = [s for (s, _), (at, n) in zip(blk["ops"], S.op_spans(blk["ops"])) if at < blk["hlit"] < at + n]
    assert crossing == [symbol]


def test_code_features():
    assert max(BLOCKS["code_of_15_bits"][0]["lit_lens"]) == 15
    one = BLOCKS["single_1_bit_distance_code"][0]
    assert sorted(l for l in one["dist_lens"] if l) == [1]
    none = BLOCKS["hdist_0_zero_length"][0]
    assert none["hdist"] == 1 and none["dist_lens"] == [0]
    assert BLOCKS["empty_final_stored_block"][-1] == S.stored(b"")
    for name in ("stored_after_unaligned_fixed", "stored_after_unaligned_dynamic"):       # the Huffman block ends inside a byte
        assert BLOCKS[name][1]["type"] == "stored" and S.deflate_bits(BLOCKS[name][:1]).bits % 8 != 0


def test_output_sizes():
    sizes = {want for _, _, want in VALID}
    assert {0, 1, 32767, 32768, 32769, 65541} <= sizes


def test_block_types_of_the_cases():
    assert {first_block_type(s) for _, s, _ in VALID} == {0, 1, 2}


def test_run_ops_round_trip():
    lens = [5] * 27 + [0] * 229 + [5] * 9 + [2, 2, 2, 3] + [0] * 4 + [7]
    out = []
    for (s, x), (at, n) in zip(S.run_ops(lens), S.op_spans(S.run_ops(lens))):
        assert at == len(out)
        out += [s] if s < 16 else [out[-1]] * n if s == 16 else [0] * n
    assert out == lens
