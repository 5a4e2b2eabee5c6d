"""zlib streams built bit by bit (RFC 1950 / 1951), in the spirit of tests/jpeg_synth.py: a stream is a list of blocks -- stored, fixed
Huffman or dynamic Huffman with given (or derived) code lengths -- of tokens, so that every corner of an inflate can be reached on
purpose: lengths and distances zlib's compressor never emits, code sets it never builds, and streams that are wrong in one place.

    tokens      ("lit", byte)   ("match", length, distance)
                ("bits", value, n)                     n raw bits, value's bit 0 first
                ("sym", s)                             literal/length symbol s with its code, nothing else (286 / 287)
                ("rawmatch", lsym, lextra, dsym, dextra)   the four fields of a match as they are
    blocks      stored(data)   fixed(tokens)   dynamic(tokens, lit_lens=, dist_lens=, cl_lens=, ops=, hlit=, hdist=, hclen=)
    zstream(blocks, ...)        the stream;  expand(blocks): what it decodes to (the builder's own, independent reading of the tokens)
    valid_cases() / invalid_cases()     the lists tests/test_inflate_host.py and tests/test_gpu_inflate.py run: (name, stream, want) with
                `want` the size of the slot the output must fill exactly; tests/test_deflate_synth.py checks them against zlib
    accepts(stream, want)       the oracle: the rule of exr.read_payload (decompressobj().decompress(stream, want + 1), eof, the length)

    python tests/deflate_synth.py --dump DIR     writes every case as DIR/<name>.<want>.zz for tools/inflate_sweep.cpp
"""
import heapq
import os
import sys
import zlib

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    """values go in from their bit 0, bytes fill from their bit 0; Huffman codes go in from their top bit"""

    def __init__(self):
        self.out, self.acc, self.cnt = bytearray(), 0, 0

    def put(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.cnt -= 8

    def code(self, code, n):
        self.put(int(format(code & ((1 << n) - 1), "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.cnt:
            self.put(0, 8 - self.cnt)

    @property
    def bits(self):
        return 8 * len(self.out) + self.cnt

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical_codes(lens):
    """RFC 1951 3.2.2, without judging the lengths (an over-subscribed set gets codes that overflow their length)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = []
    for l in lens:
        codes.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return codes


def huffman_lengths(freq, limit):
    """code lengths <= limit of the symbols with freq > 0 (a complete code when two or more occur, length 1 for one alone)"""
    used = [s for s, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    w = {s: freq[s] for s in used}
    while used:
        heap = [(w[s], s, None, None) for s in used]
        heapq.heapify(heap)
        tick = len(freq)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            heapq.heappush(heap, (a[0] + b[0], tick, a, b))
            tick += 1
        stack, deepest = [(heap[0], 0)], 0
        while stack:
            (_, s, a, b), d = stack.pop()
            if a is None:
                lens[s] = d
                deepest = max(deepest, d)
            else:
                stack += [(a, d + 1), (b, d + 1)]
        if deepest <= limit:
            break
        w = {s: (v + 1) >> 1 for s, v in w.items()}
    return lens


def length_fields(length):
    i = max(k for k in range(29) if LENGTH_BASE[k] <= length)
    return 257 + i, length - LENGTH_BASE[i]


def distance_fields(dist):
    i = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return i, dist - DIST_BASE[i]


def token_symbols(tokens):
    """(literal/length symbols, distance symbols) the tokens use"""
    lit, dist = [], []
    for t in tokens:
        if t[0] == "lit":
            lit.append(t[1])
        elif t[0] == "sym":
            lit.append(t[1])
        elif t[0] == "match":
            lit.append(length_fields(t[1])[0])
            dist.append(distance_fields(t[2])[0])
        elif t[0] == "rawmatch":
            lit.append(t[1])
            dist.append(t[3])
    return lit, dist


def stored(data):
    return {"type": "stored", "data": bytes(data)}


def fixed(tokens, eob=True):
    return {"type": "fixed", "tokens": list(tokens), "eob": eob}


def dynamic(tokens, lit_lens=None, dist_lens=None, cl_lens=None, ops=None, hlit=None, hdist=None, hclen=None, eob=True):
    """lit_lens / dist_lens: the code lengths (default: a Huffman code of the symbols the tokens use, with end-of-block; no distance
    code at all -- HDIST = 0, one length of 0 -- when there is no match); cl_lens: the 19 lengths of the code-length code; ops: the
    coded lengths as [(code-length symbol, extra value)] (default: run_ops of the concatenated lengths); hlit / hdist / hclen: the
    counts as the header states them"""
    tokens = list(tokens)
    lit_used, dist_used = token_symbols(tokens)
    if lit_lens is None:
        freq = [0] * 286
        for s in lit_used + [256]:
            freq[s] += 1
        if sum(1 for f in freq if f) < 2:
            freq[0] += 1                                            # a complete code needs two symbols
        lit_lens = huffman_lengths(freq, 15)
    if dist_lens is None:
        freq = [0] * 30
        for s in dist_used:
            freq[s] += 1
        dist_lens = huffman_lengths(freq, 15) if dist_used else [0]
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    if hlit is None:
        hlit = max(257, max([i + 1 for i, l in enumerate(lit_lens) if l] + [0]))
    if hdist is None:
        hdist = max(1, max([i + 1 for i, l in enumerate(dist_lens) if l] + [0]))
    lit_lens = (lit_lens + [0] * 288)[:hlit]
    dist_lens = (dist_lens + [0] * 32)[:hdist]
    if ops is None:
        ops = run_ops(lit_lens + dist_lens)
    if cl_lens is None:
        freq = [0] * 19
        for s, _ in ops:
            freq[s] += 1
        if sum(1 for f in freq if f) < 2:
            freq[0 if not freq[0] else 1] += 1                      # the code-length code may never be incomplete
        cl_lens = huffman_lengths(freq, 7)
    if hclen is None:
        hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
    return {"type": "dynamic", "tokens": tokens, "lit_lens": lit_lens, "dist_lens": dist_lens, "cl_lens": list(cl_lens), "ops": list(ops),
            "hlit": hlit, "hdist": hdist, "hclen": hclen, "eob": eob}


def run_ops(lens):
    """the lengths as code-length symbols, greedily run-length coded (16: repeat the previous 3..6 times, 17 / 18: 3..10 / 11..138
    zeros), over the whole list: a run does not care where the literal/length lengths end and the distance lengths begin"""
    ops, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            take = min(run, 138)
            ops.append((18, take - 11) if take >= 11 else (17, take - 3))
            i += take
        elif v and run >= 4:
            ops.append((v, 0))
            take = min(run - 1, 6)
            ops.append((16, take - 3))
            i += 1 + take
        else:
            ops.append((v, 0))
            i += 1
    return ops


def op_spans(ops):
    """[(first index, count)] of the lengths every op writes"""
    spans, at = [], 0
    for s, x in ops:
        n = 1 if s < 16 else x + 3 if s in (16, 17) else x + 11
        spans.append((at, n))
        at += n
    return spans


def _emit_tokens(w, tokens, lit_lens, dist_lens, eob):
    lit_codes, dist_codes = canonical_codes(lit_lens), canonical_codes(dist_lens)
    lit_lens, dist_lens = list(lit_lens) + [0] * 288, list(dist_lens) + [0] * 32
    lit_codes, dist_codes = lit_codes + [0] * 288, dist_codes + [0] * 32
    for t in tokens:
        if t[0] == "lit":
            w.code(lit_codes[t[1]], lit_lens[t[1]])
        elif t[0] == "sym":
            w.code(lit_codes[t[1]], lit_lens[t[1]])
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            if t[0] == "match":
                ls, lx = length_fields(t[1])
                ds, dx = distance_fields(t[2])
            else:
                _, ls, lx, ds, dx = t
            w.code(lit_codes[ls], lit_lens[ls])
            w.put(lx, LENGTH_EXTRA[ls - 257] if ls - 257 < 29 else 0)
            w.code(dist_codes[ds], dist_lens[ds])
            w.put(dx, DIST_EXTRA[ds] if ds < 30 else 0)
    if eob:
        w.code(lit_codes[256], lit_lens[256])


def deflate_bits(blocks, w=None, btypes=None):
    """the blocks into a BitWriter (the last one is final); btypes: {block index: BTYPE to state instead}"""
    w = w or BitWriter()
    for i, blk in enumerate(blocks):
        final = 1 if i == len(blocks) - 1 else 0
        w.put(final, 1)
        kind = blk["type"]
        w.put((btypes or {}).get(i, {"stored": 0, "fixed": 1, "dynamic": 2}[kind]), 2)
        if kind == "stored":
            w.align()
            n = blk.get("len", len(blk["data"]))
            w.put(n, 16)
            w.put(blk.get("nlen", n ^ 0xFFFF), 16)
            w.out += blk["data"]
        elif kind == "fixed":
            _emit_tokens(w, blk["tokens"], FIXED_LIT, FIXED_DIST, blk["eob"])
        else:
            w.put(blk["hlit"] - 257, 5)
            w.put(blk["hdist"] - 1, 5)
            w.put(blk["hclen"] - 4, 4)
            for k in range(blk["hclen"]):
                w.put(blk["cl_lens"][CL_ORDER[k]], 3)
            cl_codes = canonical_codes(blk["cl_lens"])
            for s, x in blk["ops"]:
                w.code(cl_codes[s], blk["cl_lens"][s])
                w.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
            _emit_tokens(w, blk["tokens"], blk["lit_lens"], blk["dist_lens"], blk["eob"])
    return w


def expand(blocks):
    """what the blocks decode to, read off the tokens, as far as they make sense (a stream with "bits" / "sym" tokens is not valid)"""
    out = bytearray()
    for blk in blocks:
        if blk["type"] == "stored":
            out += blk["data"]
            continue
        for t in blk["tokens"]:
            if t[0] == "lit":
                out.append(t[1])
            elif t[0] in ("match", "rawmatch"):
                if t[0] == "rawmatch":
                    if t[1] >= 286 or t[3] >= 30:
                        return bytes(out)
                    length, dist = LENGTH_BASE[t[1] - 257] + t[2], DIST_BASE[t[3]] + t[4]
                else:
                    _, length, dist = t
                if dist > len(out):
                    return bytes(out)
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out)


def zstream(blocks, cmf=0x78, flg=None, adler=None, tail=b"", btypes=None):
    """cmf flg | the blocks | Adler-32 (of expand(blocks) unless given) | tail"""
    if flg is None:
        flg = (31 - (cmf << 8) % 31) % 31
    if adler is None:
        adler = zlib.adler32(expand(blocks))
    return bytes([cmf, flg]) + deflate_bits(blocks, btypes=btypes).bytes() + adler.to_bytes(4, "big") + tail


def accepts(stream, want):
    """exr.read_payload's rule for a chunk whose scanlines hold `want` bytes"""
    d = zlib.decompressobj()
    try:
        buf = d.decompress(stream, want + 1)
    except zlib.error:
        return False
    return len(buf) == want and d.eof


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def noise(n, seed=1):
    """n literal tokens of a small generator's bytes"""
    out, x = [], seed * 2654435761 & 0xFFFFFFFF
    for _ in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(("lit", x >> 24))
    return out


def _valid_blocks():
    cases = {}
    every_length = noise(300) + [("match", L, 1 + (L * 37) % 290) for L in range(3, 259)]
    cases["every_length_fixed"] = [fixed(every_length)]
    cases["every_length_dynamic"] = [dynamic(every_length)]
    every_dist = noise(32768, 2)
    for s in range(30):
        every_dist += [("match", 3 + s % 5, DIST_BASE[s]), ("match", 4, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1)]
    cases["every_distance_fixed"] = [fixed(every_dist)]
    cases["every_distance_dynamic"] = [dynamic(every_dist)]
    overlaps = noise(70, 3)
    for D in (1, 2, 3, 63, 64, 65):
        for L in (3, 63, 64, 65, 128, 129, 258):
            if D < L:
                overlaps += [("match", L, D), ("lit", D), ("lit", L & 255)]
    cases["overlaps_fixed"] = [fixed(overlaps)]
    cases["overlaps_dynamic"] = [dynamic(overlaps)]
    cases["length_258_as_284_extra_31"] = [fixed(noise(10, 4) + [("rawmatch", 284, 31, 2, 0), ("lit", 9)])]
    # lengths 1, 2, ... 14, 15, 15: a complete code whose last two symbols have 15 bits
    lens15 = [0] * 257
    for s in range(14):
        lens15[s] = s + 1
    lens15[65], lens15[256] = 15, 15
    cases["code_of_15_bits"] = [dynamic([("lit", 65), ("lit", 0), ("lit", 13), ("lit", 65), ("lit", 12), ("lit", 1)] * 3, lit_lens=lens15)]
    cases["single_1_bit_distance_code"] = [dynamic(noise(5, 5) + [("match", 4, 3), ("lit", 1), ("match", 30, 3)])]
    cases["single_1_bit_literal_code"] = [dynamic([], lit_lens=[0] * 256 + [1])]
    cases["hdist_0_zero_length"] = [dynamic(noise(200, 6))]
    # a run of 16 over the boundary: 32 codes of 5 bits (27 literals, 256 .. 260), then distance lengths that go on with 5s
    lit5 = [5] * 27 + [0] * 229 + [5] * 5
    cases["run_16_crosses_boundary"] = [dynamic([("lit", 3), ("match", 4, 1), ("lit", 26), ("match", 5, 4)], lit_lens=lit5,
                                                dist_lens=[5, 5, 5, 5, 2, 2, 2, 3])]
    few = huffman_lengths([1 if s < 10 or s in (256, 257) else 0 for s in range(258)], 15)      # literals 0 .. 9, length 3
    pi = [("lit", v) for v in (3, 1, 4, 1, 5, 9, 2, 6, 5)]
    cases["run_17_crosses_boundary"] = [dynamic(pi + [("match", 3, 4), ("match", 3, 5), ("lit", 2)], lit_lens=few + [0], hlit=259,
                                                dist_lens=[0, 0, 0, 1, 1], hdist=5)]
    cases["run_18_crosses_boundary"] = [dynamic(pi + [("match", 3, 7), ("match", 3, 9), ("lit", 2)], lit_lens=few + [0] * 13, hlit=271,
                                                dist_lens=[0, 0, 0, 0, 0, 1, 1], hdist=7)]
    cases["empty_final_stored_block"] = [fixed(noise(20, 7)), stored(b"")]
    cases["stored_after_unaligned_fixed"] = [fixed(noise(5, 8)), stored(b"stored bytes after a block that ends inside a byte"), fixed(noise(3, 9))]
    cases["stored_after_unaligned_dynamic"] = [dynamic(noise(40, 10)), stored(bytes(range(256)) * 3)]
    cases["match_across_blocks_and_types"] = [stored(bytes(range(100, 200))), fixed([("match", 50, 80), ("lit", 1)]),
                                              dynamic([("match", 100, 140), ("lit", 2), ("match", 258, 151)]),
                                              stored(b"xyz"), fixed([("match", 9, 3), ("match", 200, 412)])]
    cases["several_dynamic_blocks"] = [dynamic(noise(100, 11)), dynamic(noise(50, 12) + [("match", 20, 120)]), dynamic([("match", 3, 1)])]
    cases["stored_65535"] = [stored(bytes(k * 7 & 255 for k in range(65535))), stored(b"\x01\x02")]
    cases["output_0_fixed"] = [fixed([])]
    cases["output_0_stored"] = [stored(b"")]
    cases["output_1"] = [fixed([("lit", 0xA5)])]

    def long_tokens(total, seed):
        """1000 literals, then matches of 258 at changing distances with a literal between them, to `total` bytes exactly"""
        toks, n, k = noise(1000, seed), 1000, 0
        while total - n >= 259:
            toks += [("match", 258, 1 + (k * 131) % min(n, 32768)), ("lit", k & 255)]
            n += 259
            k += 1
        return toks + noise(total - n, seed + 1)

    for total in (32767, 32768, 32769):
        cases["output_%d" % total] = [dynamic(long_tokens(total, total))]
    cases["match_straddles_32768"] = [fixed(noise(32700, 13) + [("match", 69, 32700)])]
    wrap = noise(32768, 14) + [("match", 258, 32768)] * 126 + [("match", 200, 32768), ("match", 65, 3)]
    cases["output_65541_distance_32768"] = [fixed(wrap)]
    cases["output_65541_dynamic"] = [dynamic(wrap[:20000]), dynamic(wrap[20000:])]
    return cases


def valid_cases():
    """[(name, stream, want)]: zlib accepts every one, and decodes it to expand() of its blocks"""
    out = []
    for name, blocks in _valid_blocks().items():
        out.append((name, zstream(blocks), len(expand(blocks))))
    blocks = [fixed(noise(30, 20))]
    out.append(("trailing_bytes", zstream(blocks, tail=b"\x00\xffmore"), 30))
    out.append(("cinfo_0", zstream(blocks, cmf=0x08), 30))
    return out


def invalid_cases():
    """[(name, stream, want)]: one per way to be wrong; the oracle refuses every one"""
    lits = noise(30, 21)
    good = zstream([fixed(lits)])
    out = [("empty_input", b"", 0),
           ("truncated_in_zlib_header", good[:1], 30),
           ("cm_7", zstream([fixed(lits)], cmf=0x77), 30),
           ("cinfo_8", zstream([fixed(lits)], cmf=0x88), 30),
           ("header_check", zstream([fixed(lits)], flg=((31 - (0x78 << 8) % 31) % 31) ^ 1), 30),
           ("fdict", zstream([fixed(lits)], flg=0x20 + (31 - ((0x78 << 8) + 0x20) % 31) % 31), 30),
           ("block_type_3", zstream([fixed(lits)], btypes={0: 3}), 30),
           ("stored_nlen", zstream([dict(stored(b"abcdef"), nlen=0x1234)]), 6),
           ("stored_truncated", zstream([stored(b"abcdef")])[:9], 6),
           ("wrong_adler", zstream([fixed(lits)], adler=zlib.adler32(expand([fixed(lits)])) ^ 0x100), 30),
           ("output_one_longer_than_slot", good, 29),
           ("output_one_shorter_than_slot", good, 31),
           ("stored_longer_than_slot", zstream([stored(b"abcdef")]), 5)]
    for cut in (1, 2, 3, 4):
        out.append(("truncated_in_adler_%d" % cut, good[:-cut], 30))
    out.append(("truncated_in_a_code", good[:14], 30))
    dyn = zstream([dynamic(noise(100, 22) + [("match", 10, 50)])])
    for cut in (3, 5, 12, 30):
        out.append(("truncated_in_dynamic_header_%d" % cut, dyn[:cut], 110))
    toks = noise(10, 23)
    lit_lens = dynamic(toks)["lit_lens"]

    def dyn_case(name, want=10, **kw):
        out.append((name, zstream([dynamic(kw.pop("tokens", toks), **kw)]), want))

    dyn_case("hlit_287", lit_lens=lit_lens + [0] * 30, hlit=287)
    dyn_case("hlit_288", lit_lens=lit_lens + [0] * 31, hlit=288)
    dyn_case("hdist_31", dist_lens=[0] * 31, hdist=31)
    dyn_case("hdist_32", dist_lens=[0] * 32, hdist=32)
    cl = dynamic(toks)["cl_lens"]
    over = list(cl)
    over[[s for s in range(19) if cl[s]][0]] = 1
    over[[s for s in range(19) if cl[s]][1]] = 1
    over[[s for s in range(19) if cl[s]][2]] = 1
    dyn_case("code_length_code_oversubscribed", cl_lens=over)
    dyn_case("code_length_code_incomplete", cl_lens=[l + 1 if l else 0 for l in cl])
    dyn_case("code_length_code_single", tokens=[], lit_lens=[1] * 257, ops=[(1, 0)] * 258, cl_lens=[0, 1] + [0] * 17, dist_lens=[1], want=0)
    dyn_case("code_length_code_empty", cl_lens=[0] * 19, hclen=19)
    ops = run_ops(dynamic(toks)["lit_lens"] + [0])
    dyn_case("repeat_16_first", ops=[(16, 0)] + ops, cl_lens=huffman_lengths([1 if s in {o for o, _ in ops} | {16} else 0 for s in range(19)], 7))
    dyn_case("run_overflows", ops=ops[:-1] + [(18, 127)], cl_lens=huffman_lengths([1 if s in {o for o, _ in ops} | {18} else 0 for s in range(19)], 7))
    no_eob = list(lit_lens)
    no_eob[256] = 0
    dyn_case("no_end_of_block", lit_lens=no_eob + [lit_lens[256]], eob=False)
    dyn_case("literal_set_oversubscribed", tokens=[], lit_lens=[1, 1] + [0] * 254 + [1], want=0)
    dyn_case("literal_set_incomplete", tokens=[], lit_lens=[1] + [0] * 255 + [2], want=0)
    dyn_case("distance_set_oversubscribed", tokens=[], dist_lens=[1, 1, 1], want=0)
    dyn_case("distance_set_incomplete", tokens=[], dist_lens=[2, 2], want=0)
    dyn_case("unassigned_literal_code", tokens=[("bits", 1, 1)], lit_lens=[0] * 256 + [1], want=0)
    dyn_case("unassigned_distance_code", tokens=toks + [("sym", 257), ("bits", 1, 1)],
             lit_lens=huffman_lengths([1 if s in {t[1] for t in toks} | {256, 257} else 0 for s in range(258)], 15), dist_lens=[1], want=13)
    dyn_case("match_without_distance_codes", tokens=toks + [("sym", 257), ("bits", 0, 1)],
             lit_lens=huffman_lengths([1 if s in {t[1] for t in toks} | {256, 257} else 0 for s in range(258)], 15), dist_lens=[0], want=13)
    out.append(("literal_symbol_286", zstream([fixed(lits + [("sym", 286)])]), 30))
    out.append(("literal_symbol_287", zstream([fixed(lits + [("sym", 287)])]), 30))
    out.append(("distance_symbol_30", zstream([fixed(lits + [("rawmatch", 257, 0, 30, 0)])]), 33))
    out.append(("distance_symbol_31", zstream([fixed(lits + [("rawmatch", 257, 0, 31, 0)])]), 33))
    out.append(("distance_before_first_byte", zstream([fixed([("match", 3, 1)])]), 3))
    out.append(("distance_too_far_back", zstream([fixed(lits[:4] + [("match", 3, 5)])]), 7))
    out.append(("distance_too_far_back_dynamic", zstream([dynamic(lits + [("match", 3, 31)])]), 33))
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--dump":
        sys.exit(__doc__)
    os.makedirs(sys.argv[2], exist_ok=True)
    for name, stream, want in valid_cases() + invalid_cases():
        with open(os.path.join(sys.argv[2], "%s.%d.zz" % (name, want)), "wb") as f:
            f.write(stream)
    print("%d streams in %s" % (len(valid_cases() + invalid_cases()), sys.argv[2]))
