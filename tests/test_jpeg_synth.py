"""The synthetic JPEG files of tests/jpeg_synth.py, on the host: the writer round-trips through the sequential reference
(tests/jpeg_ref.py), the reference's pixels equal PIL's on every case the device test compares pixels on (that is what licenses
its `pixels` flag), jpeg.parse / jpeg.plan read the files as the writer's arguments say, the tables the kernel is given decode
every code of every Huffman table used, and the model of jpeg_sync_kernel ends on the sequential chain."""
import numpy as np
import pytest

import jpeg_ref
import jpeg_synth
from jpeg_synth import CASES

BY_NAME = {c.name: c for c in CASES}
ACCEPTED = [c for c in CASES if c.refused is None]
SYNTHETIC = [c for c in ACCEPTED if c.args is not None]
ZERO_STREAMS = [c for c in CASES if c.zero_stream]
ids = lambda cases: [c.name for c in cases]


@pytest.fixture(scope="module")
def jpeg(shdr):
    return shdr.jpeg


def test_case_list_is_what_the_device_test_relies_on():
    assert tuple(c.name for c in CASES if not c.pixels) == jpeg_synth.EXTREME == ("extreme-dense-1023-444", "extreme-dqt-65535-grey")
    small = [c for c in CASES if c.small]
    assert len(small) > 64                                                # a batch of them crosses jpeg_errors_kernel's 64-thread block
    for c in small:
        hd = jpeg_ref.markers(c.data)
        assert hd["width"] <= 64 and hd["height"] <= 64, c.name
    assert len(ZERO_STREAMS) == 3 and {c.refused for c in CASES if c.group == "refused"} == {"more than four Huffman tables", "sampling factors"}
    # chroma planes 1, 2 and 3 wide, 1 and 2 high, in both subsampled layouts: both sides of libjpeg's cw > 2 switch
    for layout in ("422", "420"):
        planes = {jpeg_ref.grid(jpeg_ref.markers(c.data))[2][1][4:] for c in CASES if c.group == "layout" and "-%s-" % layout in c.name}
        assert {cw for cw, _ in planes} >= {1, 2, 3} and {ch for _, ch in planes} >= {1, 2}, (layout, planes)
        assert (3, 1) in planes and (2, 1) in planes


@pytest.mark.parametrize("case", SYNTHETIC, ids=ids(SYNTHETIC))
def test_reference_returns_the_writers_input(case):
    _, coef = jpeg_ref.coefficients(case.data)
    assert len(coef) == len(case.coef)
    for c, (got, want) in enumerate(zip(coef, case.coef)):
        assert got.shape == want.shape and np.array_equal(got, want), (case.name, c)


@pytest.mark.parametrize("case", [c for c in ACCEPTED if c.pixels], ids=ids([c for c in ACCEPTED if c.pixels]))
def test_reference_pixels_equal_pil(case):
    """a case that fails here is changed until it passes, or is one of the two named extreme cases: never skipped"""
    got = jpeg_ref.decode(case.data)
    assert got.shape == case.pil.shape and np.array_equal(got, case.pil), case.name


def test_the_coefficients_meant_are_in_the_files():
    """the statistics each case is named after, read back from its own input"""
    def symbols(case):                                                     # (DC categories, AC (run, size) symbols incl. ZRL / EOB)
        dc, ac = set(), set()
        a = case.args
        mx, my, grid = jpeg_synth.block_grid(a["width"], a["height"], a["comps"])
        ri = a.get("restart_interval", 0)
        for c, blocks in enumerate(a["coef"]):
            h, v = (1, 1) if len(a["comps"]) == 1 else a["comps"][c][1:3]
            pred = 0
            for i, (y, x) in enumerate(jpeg_synth.scan_order(blocks.shape[0], blocks.shape[1], h, v)):
                if ri and (i // (h * v)) % ri == 0 and i % (h * v) == 0:
                    pred = 0
                zz = blocks[y, x][jpeg_ref.ZZ].astype(int)
                dc.add(abs(int(zz[0]) - pred).bit_length())
                pred = int(zz[0])
                nz = np.flatnonzero(zz[1:]) + 1
                prev = 0
                for k in nz:
                    run = k - prev - 1
                    ac.update(["ZRL"] * (run // 16))
                    ac.add((int(run % 16), abs(int(zz[k])).bit_length()))
                    prev = k
                ac.add("EOB" if prev != 63 else "no EOB")
        return dc, ac
    dc, ac = symbols(BY_NAME["dc-category-11-444"])
    assert dc == {11} and ac == {"EOB"}                                    # differences of -1024, then +-2047; EOB-only blocks
    assert symbols(BY_NAME["dc-category-11-restart-1-444"])[0] == {10, 11}  # the predictor resets: -1024 and +1023 themselves
    assert 11 in symbols(BY_NAME["dc-category-11-restart-1-420"])[0]
    for name in ("ac-1023-walking-grey", "ac-1023-walking-422", "ac-1023-walking-all-16-bit-444"):
        dc, ac = symbols(BY_NAME[name])
        assert {s for s in ac if isinstance(s, tuple)} == {(r, 10) for r in range(16)} and {"ZRL", "EOB", "no EOB"} <= ac, name
    for name in ("every-symbol-all-16-bit-grey", "every-symbol-9-10-boundary-444", "every-symbol-typical-444"):
        case = BY_NAME[name]                                               # every symbol of every table of the file is in its stream
        dc, ac = symbols(case)
        assert dc == set(range(12)) and ac >= {(r, s) for r in range(16) for s in range(1, 11)} | {"ZRL", "EOB"}, name
        assert all(len(symbols_) in (12, 162) for _, symbols_ in case.args["htables"].values())
    for name in ("only-zigzag-63-420", "only-zigzag-63-grey"):
        coef = BY_NAME[name].args["coef"]
        assert all(np.all(a[..., 63] != 0) and np.count_nonzero(a[..., 1:]) == a.shape[0] * a.shape[1] for a in coef)
        assert {"ZRL", "no EOB"} <= symbols(BY_NAME[name])[1] <= {"ZRL", (14, 1), (14, 2), (14, 3), "no EOB"}
    assert symbols(BY_NAME["dense-255-444"])[1] >= {"no EOB"} and "EOB" not in symbols(BY_NAME["dense-255-444"])[1]
    assert {"EOB", "no EOB"} <= symbols(BY_NAME["dense-next-to-eob-only-420"])[1] and 0 in symbols(BY_NAME["dense-next-to-eob-only-420"])[0]
    assert (0, 10) in symbols(BY_NAME["extreme-dense-1023-444"])[1]
    for c in ZERO_STREAMS:                                                 # every bit of the scan is zero: nothing to stuff, no padding
        scan = c.data[c.info["scan_start"]:c.info["scan_end"]]
        mx, my, _ = jpeg_synth.block_grid(c.args["width"], c.args["height"], c.args["comps"])
        assert scan == bytes(len(scan)) and 8 * len(scan) == mx * my * sum(c.zero_stream), c.name


@pytest.mark.parametrize("case", ACCEPTED, ids=ids(ACCEPTED))
def test_parse_reads_what_the_writer_wrote(jpeg, case):
    hd = jpeg.parse(case.data)
    if case.args is None:                                                  # written by PIL: against the reference's marker walk
        ref = jpeg_ref.markers(case.data)
        assert (hd.width, hd.height, [tuple(c) for c in hd.components]) == (ref["width"], ref["height"], ref["comps"])
        assert jpeg.geometry(hd)[3] == jpeg_ref.grid(ref)[2] and hd.rst_offsets.tolist() == ref["rst"]
        return
    a = case.args
    assert (hd.width, hd.height) == (a["width"], a["height"]) and [tuple(c) for c in hd.components] == a["comps"]
    assert hd.layout == case.name.rsplit("-", 1)[1]
    assert set(hd.qtables) >= {c[3] for c in a["comps"]} and set(hd.qtables) == set(a["qtables"])
    for t, q in a["qtables"].items():
        assert hd.qtables[t].dtype == np.uint16 and hd.qtables[t].tolist() == list(q), (case.name, t)
    assert set(hd.htables) == set(a["htables"])
    for k, (counts, symbols) in a["htables"].items():
        assert (hd.htables[k][0].tolist(), hd.htables[k][1].tolist()) == (list(counts), list(symbols)), (case.name, k)
    ri = a.get("restart_interval", 0)
    assert hd.restart_interval == ri and hd.orientation == 1
    assert (hd.scan_start, hd.scan_end) == (case.info["scan_start"], case.info["scan_end"])
    assert hd.rst_offsets.tolist() == case.info["rst_offsets"]
    mx, my, grid = jpeg_synth.block_grid(a["width"], a["height"], a["comps"])
    gmx, gmy, bpm, comps = jpeg.geometry(hd)
    assert (gmx, gmy) == (mx, my) and [(c[3], c[2]) for c in comps] == grid
    assert bpm == (1 if len(grid) == 1 else sum(c[1] * c[2] for c in a["comps"]))
    assert len(case.info["rst_offsets"]) == (-(-mx * my // ri) - 1 if ri else 0)
    assert [case.data[o + 1] - 0xD0 for o in case.info["rst_offsets"]] == [i % 8 for i in range(len(case.info["rst_offsets"]))]
    # the plan the device gets: one row per restart segment with its blocks, the unstuffed bytes of each on a dword boundary
    p = jpeg.plan([case.data], 256)
    per = (ri if ri else mx * my) * bpm
    assert p.segs.shape[0] == len(case.info["rst_offsets"]) + 1 and p.segs[:, 3].tolist() == [per * i for i in range(p.segs.shape[0])]
    assert p.segs[:, 4].sum() == mx * my * bpm and p.segs[:, 4].max() <= per and p.segs[:, 4].min() > 0
    segs = jpeg_ref.unstuff(case.data, jpeg_ref.markers(case.data))
    for row, seg in zip(p.segs, segs):
        assert row[1] == 8 * len(seg) and p.data[4 * row[0]:4 * row[0] + len(seg)].tobytes() == seg


def test_restart_cases_are_the_edges_they_are_named_after(jpeg):
    info = lambda name: (BY_NAME[name].args, BY_NAME[name].info, jpeg.plan([BY_NAME[name].data]))
    for name in ("restart-splits-the-mcu-row-420", "restart-splits-the-mcu-row-422"):
        a, i, p = info(name)
        mx = jpeg_synth.block_grid(a["width"], a["height"], a["comps"])[0]
        assert mx % a["restart_interval"] != 0 and len(i["rst_offsets"]) >= 2
    a, i, p = info("restart-equals-the-mcus-420")
    assert a["restart_interval"] == 12 == p.images["mcus_x"][0] * p.images["mcus_y"][0] and i["rst_offsets"] == [] and p.segs.shape[0] == 1
    a, i, p = info("restart-larger-than-the-mcus-420")
    assert a["restart_interval"] > p.images["mcus_x"][0] * p.images["mcus_y"][0] and i["rst_offsets"] == [] and p.segs[0, 4] == 12 * 6
    assert info("restart-35-segments-grey")[2].segs.shape[0] == 35 and info("restart-15-segments-444")[2].segs.shape[0] == 15


def test_one_dht_segment_or_one_each(jpeg):
    a, b = BY_NAME["dht-one-segment-420"], BY_NAME["dht-segment-each-420"]
    assert a.data.count(b"\xff\xc4") == 1 and b.data.count(b"\xff\xc4") == 4 and len(a.data) == len(b.data) - 12
    ha, hb = jpeg.parse(a.data), jpeg.parse(b.data)
    assert set(ha.htables) == set(hb.htables) and all(np.array_equal(x, y) for k in ha.htables for x, y in zip(ha.htables[k], hb.htables[k]))
    assert a.data[ha.scan_start:] == b.data[hb.scan_start:]


def test_out_of_scope_files_are_refused(jpeg):
    with pytest.raises(jpeg.Unsupported, match="sampling factors 1x2/1x1/1x1"):                     # 4:4:0
        jpeg.parse(BY_NAME["sampling-440"].data)
    five = BY_NAME["huff-five-tables-444"]
    assert len(jpeg.parse(five.data).htables) == 5                          # a legal file: the container is fine
    with pytest.raises(jpeg.Unsupported, match="more than four Huffman tables"):
        jpeg.plan([five.data])
    with pytest.raises(jpeg.Unsupported, match="bytes>.*more than four"):   # in a batch, naming the item
        jpeg.plan([BY_NAME["sof1-420"].data, five.data])
    four = jpeg.plan([BY_NAME["huff-four-slots-444"].data])
    assert sorted({int(four.images["comp"][0][c][k]) for c in range(3) for k in ("dc_slot", "ac_slot")}) == [0, 1, 2, 3]
    assert len({int(four.images["comp"][0][c]["ac_slot"]) for c in range(3)}) == 3


def _tables():
    seen = {}
    for c in SYNTHETIC:
        for key, (counts, symbols) in c.args["htables"].items():
            seen.setdefault((tuple(counts), tuple(symbols)), "%s %s%d" % (c.name, "AC" if key[0] else "DC", key[1]))
    return sorted((name, counts, symbols) for (counts, symbols), name in seen.items())


@pytest.mark.parametrize("name,counts,symbols", _tables(), ids=[t[0] for t in _tables()])
def test_device_huffman_tables_decode_every_code(jpeg, name, counts, symbols):
    """decode_run's symbol lookup (csrc/jpeg.hip), read in Python over the tables jpeg.device_huffman gives it: every code of every
    table used here, followed by zeros and by ones, comes back with its length and symbol; a peek no code starts is refused"""
    blob = jpeg.device_huffman(np.array(counts, dtype=np.uint8), np.array(symbols, dtype=np.uint8))
    look = blob[:1024].view(np.uint16)
    maxcode, valoff, val = blob[1024:1092].view(np.int32), blob[1092:1160].view(np.int32), blob[1160:]

    def lookup(v):                                                         # v: the next 32 bits of the stream
        e = int(look[v >> 23])
        if e:
            return e >> 8, e & 255
        n, code = 10, v >> 22
        while n <= 16 and code > maxcode[n]:
            n += 1
            code = v >> (32 - n)
        return (n, int(val[(code + valoff[n]) & 255])) if n <= 16 else None

    book = jpeg_ref.code_book(list(counts), list(symbols))
    assert len(book) == len(symbols) == sum(counts)
    for (l, code), sym in book.items():
        for tail in (0, (1 << (32 - l)) - 1, 0x5A5A5A5A & ((1 << (32 - l)) - 1)):
            assert lookup(code << (32 - l) | tail) == (l, sym), (name, l, code)
    top = max(l for l, _ in book)
    last = max(c for l, c in book if l == top)
    if (last + 1) << (16 - top) < 1 << 16:                                  # an incomplete code: what follows the last code is none
        assert lookup(((last + 1) << (32 - top)) & 0xFFFFFFFF) is None and lookup(0xFFFFFFFF) is None
    if top <= 9:
        assert np.all(look[(last + 1) << (9 - top):] == 0)


def test_tables_cover_what_the_issue_names():
    lengths = {name: {l + 1 for l, n in enumerate(counts) if n} for name, counts, symbols in _tables()}
    assert {16} in lengths.values() and {10} in lengths.values() and {9, 10} in lengths.values() and {1} in lengths.values()
    assert any(len(symbols) == 1 for _, _, symbols in _tables()) and any(len(symbols) == 162 and min(l) == 16 for (_, _, symbols), l in
                                                                        zip(_tables(), lengths.values()))


@pytest.mark.parametrize("bits", [256, 512, 1024, 2048])
@pytest.mark.parametrize("case", ZERO_STREAMS, ids=ids(ZERO_STREAMS))
def test_sync_model_ends_on_the_sequential_chain(case, bits):
    """sync_model asserts it itself; here also what makes these streams the worst case: a pass per workgroup"""
    a = case.args
    mx, my, _ = jpeg_synth.block_grid(a["width"], a["height"], a["comps"])
    m = jpeg_synth.sync_model(case.zero_stream, mx * my, bits, detail=True)
    assert m.passes == jpeg_synth.sync_model(case.zero_stream, mx * my, bits)
    assert m.workgroups == -(-(-(-mx * my * sum(case.zero_stream) // bits)) // jpeg_synth.WG)
    assert m.passes == max(2, m.workgroups) and len(m.iterations) == m.passes
    if m.workgroups > 2:                                                   # the in-workgroup loop runs to its cap of WG + 1 iterations
        assert max(m.iterations) == jpeg_synth.WG + 1
    assert m.rounds.max() // (jpeg_synth.WG + 2) == (m.passes - 1 if m.workgroups > 1 else 0)
    if bits == 256:
        assert m.passes >= 5


def test_sync_model_of_the_issues_stream():
    """4:2:2, 24 x 16 MCUs of 697 bits at 256 bits per subsequence: five workgroups, five passes"""
    m = jpeg_synth.sync_model((127, 127, 190, 253), 24 * 16, 256, detail=True)
    assert (m.passes, m.workgroups, m.iterations) == (5, 5, [256, 257, 257, 257, 23])


def test_noise_file_segments_straddle_workgroups(jpeg):
    """the PIL-written restart file at 256 bits: a workgroup that starts inside a segment, and one that holds two segments"""
    p = jpeg.plan([BY_NAME["noise-256x384-restart-40-420"].data], 256)
    by_wg = p.sub_seg.reshape(-1, jpeg.WG)
    assert p.segs.shape[0] == 10 and by_wg.shape[0] >= 4
    assert any(wg > 0 and by_wg[wg, 0] == by_wg[wg - 1, -1] for wg in range(by_wg.shape[0]))
    assert any(len(set(row[row >= 0].tolist())) >= 2 for row in by_wg)
    for name in ("flat-white-1024x2048-grey", "flat-mid-grey-1024x2048-grey"):
        assert jpeg.plan([BY_NAME[name].data], 256).images["n_wg"][0] >= 3
