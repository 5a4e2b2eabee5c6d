"""CPU tests of the happens-before auditor (tests/stream_audit.py): the checker on hand-written logs, the aten recorder on CPU tensors
with stand-in stream ids, the header parser on include/shdr.h."""
import importlib

import pytest
import torch

import stream_audit as SA

A, B = (0x1000, 0x1100), (0x2000, 0x2100)


def W(name, stream, *ivs):
    return ("launch", name, stream, [], list(ivs))


def R(name, stream, *ivs):
    return ("launch", name, stream, list(ivs), [])


def run(*log):
    return SA.Checker().run(log)


# ---- the checker on hand-written logs ----------------------------------------------------------------------------------------------------
PLANTED = {"write->read": (W("produce", 1, A), R("consume", 2, A)),
           "read->write": (R("consume", 1, A), W("overwrite", 2, A)),
           "write->write": (W("produce", 1, A), W("overwrite", 2, A))}


@pytest.mark.parametrize("kind", sorted(PLANTED))
def test_planted_conflict_is_reported_naming_both_sides(kind):
    first, second = PLANTED[kind]
    ck = run(first, second)
    assert len(ck.reports) == 1 and (ck.examined, ck.ordered) == (1, 0)
    r = ck.reports[0]
    assert r.kind == kind and (r.first.name, r.first.stream, r.first.idx) == (first[1], 1, 0)
    assert (r.second.name, r.second.stream, r.second.idx) == (second[1], 2, 1) and (r.lo, r.hi) == A
    line = r.line()
    assert first[1] in line and second[1] in line and "stream 1" in line and "stream 2" in line and kind in line


ORDERINGS = {"wait_stream": [("wait_stream", 2, 1)],
             "record + wait_event": [("record", "e", 1), ("wait_event", 2, "e")],
             "query() is True": [("record", "e", 1), ("query_true", "e")],
             "Event.synchronize": [("record", "e", 1), ("sync_event", "e")],
             "Stream.synchronize": [("sync_stream", 1)],
             "device synchronize": [("sync_all",)]}


@pytest.mark.parametrize("how", sorted(ORDERINGS))
@pytest.mark.parametrize("kind", sorted(PLANTED))
def test_each_ordering_removes_the_report(kind, how):
    first, second = PLANTED[kind]
    ck = run(first, *ORDERINGS[how], second)
    assert not ck.reports and (ck.examined, ck.ordered) == (1, 1)


def test_an_ordering_covers_only_what_was_enqueued_before_it():
    # the event is recorded BEFORE the producer: waiting for it orders nothing; so does a wait in the wrong direction
    assert len(run(("record", "e", 1), W("produce", 1, A), ("wait_event", 2, "e"), R("consume", 2, A)).reports) == 1
    assert len(run(W("produce", 1, A), ("wait_stream", 1, 2), R("consume", 2, A)).reports) == 1
    # a host synchronisation of ANOTHER stream orders nothing
    assert len(run(W("produce", 1, A), ("sync_stream", 3), R("consume", 2, A)).reports) == 1
    # work enqueued on the producer's stream after the wait is not covered by it
    ck = run(W("produce", 1, A), ("wait_stream", 2, 1), W("produce again", 1, A), R("consume", 2, A))
    assert len(ck.reports) == 1 and ck.reports[0].first.name == "produce again"


def test_ordering_is_transitive_over_three_streams():
    ck = run(W("produce", 1, A), ("wait_stream", 2, 1), W("other", 2, B), ("wait_stream", 3, 2), R("consume", 3, A))
    assert not ck.reports and ck.ordered == 1
    # ... and through the host: stream 2 waited for 1, the host for 2
    assert not run(W("produce", 1, A), ("wait_stream", 2, 1), ("sync_stream", 2), R("consume", 3, A)).reports
    # not transitive backwards
    assert len(run(W("produce", 1, A), ("wait_stream", 3, 2), ("wait_stream", 2, 1), R("consume", 3, A)).reports) == 1


def test_readers_and_disjoint_writers_do_not_conflict():
    ck = run(W("init", 1, A), ("sync_all",), R("read", 1, A), R("read", 2, A), R("read", 3, A))
    assert not ck.reports
    lo = A[0]
    ck = run(W("left", 1, (lo, lo + 64)), W("right", 2, (lo + 64, lo + 128)), R("left", 1, (lo, lo + 64)), R("right", 2, (lo + 64, lo + 128)))
    assert not ck.reports and ck.examined == 0


def test_one_byte_of_overlap_is_reported():
    lo = A[0]
    ck = run(W("left", 1, (lo, lo + 65)), W("right", 2, (lo + 64, lo + 128)))
    assert len(ck.reports) == 1 and (ck.reports[0].lo, ck.reports[0].hi) == (lo + 64, lo + 65)
    assert not run(W("left", 1, (lo, lo + 64)), W("right", 2, (lo + 64, lo + 128))).reports


def test_every_reader_since_the_last_write_is_checked():
    ck = run(W("init", 0, A), ("sync_all",), R("r1", 1, A), R("r2", 2, A), ("wait_stream", 3, 1), W("overwrite", 3, A))
    assert [(r.kind, r.first.name) for r in ck.reports] == [("read->write", "r2")]


def test_segments_tile_any_sequence_of_intervals():
    import random
    rnd = random.Random(5)
    ck = SA.Checker()
    for _ in range(300):
        lo = rnd.randrange(0, 200)
        hi = lo + rnd.randrange(1, 60)
        segs = ck._cover(lo, hi)
        assert segs[0].lo == lo and segs[-1].hi == hi and all(a.hi == b.lo for a, b in zip(segs, segs[1:]))
        assert ck._starts == sorted(ck._starts) == [s.lo for s in ck._segs] and all(a.hi <= b.lo for a, b in zip(ck._segs, ck._segs[1:]))


def test_summary_counts():
    ck = run(W("a", 1, A), ("wait_stream", 2, 1), R("b", 2, A), W("c", 3, A))
    assert len(ck.launches) == 3 and ck.examined == 3 and ck.ordered == 1 and len(ck.reports) == 2       # c against a and against b
    assert "launches 3 on 3 stream(s)" in ck.summary() and "reports 2" in ck.summary()


# ---- the aten recorder on CPU tensors ---------------------------------------------------------------------------------------------------
class Streams:
    """stand-in for torch.cuda.current_stream()"""

    def __init__(self):
        self.cur = 0

    def __call__(self):
        return self.cur


@pytest.fixture
def rec():
    st = Streams()
    r = SA.Recorder(stream_of=st, all_tensors=True)
    r.on = lambda s: setattr(st, "cur", s)
    return r


def test_aten_write_then_read_across_streams(rec):
    x = torch.zeros(64)
    with rec:
        rec.on(1)
        x.add_(1.0)
        rec.on(2)
        y = x * 2.0
    ck = rec.checker
    assert not rec.errors and len(ck.reports) == 1 and ck.reports[0].kind == "write->read"
    assert (ck.reports[0].first.name, ck.reports[0].second.name) == ("aten.add_", "aten.mul") and (ck.reports[0].lo, ck.reports[0].hi) == SA.interval(x)
    assert "x" in ck.reports[0].line(SA.catalog({"t": {"x": x, "y": y}}))


def test_aten_orderings_and_host_reads(rec):
    x = torch.zeros(64)
    with rec:
        rec.on(1)
        x.add_(1.0)
        rec.checker.wait_stream(2, 1)
        rec.on(2)
        y = x * 2.0                       # ordered after the write on stream 1
        float(y.sum())                    # the host waits for stream 2 ...
        rec.on(4)
        y.zero_()                         # ... so everything enqueued from now on is ordered after stream 2's work
        assert not rec.checker.reports and rec.checker.ordered == rec.checker.examined >= 2, rec.checker.summary()
        rec.on(3)
        y.mul_(2.0)                       # reads and writes y; nothing orders stream 3 after stream 4
    kinds = [(r.kind, r.first.name, r.second.name) for r in rec.checker.reports]
    assert not rec.errors and kinds == [("write->read", "aten.zero_", "aten.mul_"), ("write->write", "aten.zero_", "aten.mul_")], kinds


def test_aten_out_argument_is_a_write(rec):
    x, out = torch.ones(8), torch.empty(8)
    with rec:
        rec.on(1)
        torch.add(x, x, out=out)
        rec.on(2)
        out.sum()
    assert [r.kind for r in rec.checker.reports] == ["write->read"]


def test_views_access_nothing(rec):
    x = torch.zeros(4, 16)
    with rec:
        rec.on(1)
        x.add_(1.0)
        n = len(rec.checker.launches)
        rec.on(2)
        views = [x.view(64), x[1], x[:, 2:4], x.detach(), x.t(), x.reshape(8, 8), x.unsqueeze(0), x.expand(4, 16), torch.split(x, 2),
                 torch.chunk(x, 2, dim=1), x.permute(1, 0), x.flatten(), x.as_strided((2, 2), (1, 1))]
        torch.empty(8)
        torch.empty_like(x)
    assert not rec.errors and len(views) == 13 and len(rec.checker.launches) == n and not rec.checker.reports


def test_disjoint_slices_of_one_storage(rec):
    flat = torch.zeros(256)                  # as FlatParams: every variable a slice of one buffer
    a, b = flat[0:64].view(8, 8), flat[64:128].view(8, 8)
    with rec:
        rec.on(1)
        a.add_(1.0)
        rec.on(2)
        b.add_(1.0)
        assert not rec.checker.reports       # byte intervals, not storages
        rec.on(3)
        flat.mul_(0.5)                       # the whole buffer: conflicts with both
    assert sorted((r.first.stream, r.kind) for r in rec.checker.reports) == [(1, "write->read"), (1, "write->write"), (2, "write->read"),
                                                                             (2, "write->write")]


def test_strided_view_spans_its_strides(rec):
    x = torch.zeros(8, 8)
    col = x[:, 3]                             # bytes of 7 rows + one element
    assert SA.interval(col) == (x.data_ptr() + 12, x.data_ptr() + 12 + (7 * 8 + 1) * 4)
    one = torch.zeros(16, dtype=torch.uint8)
    with rec:
        rec.on(1)
        one[0:9].add_(1)
        rec.on(2)
        one[8:16].add_(1)                     # one byte in common
    assert rec.checker.reports and all((r.lo, r.hi) == (one.data_ptr() + 8, one.data_ptr() + 9) for r in rec.checker.reports)


def test_capture_and_replay(rec):
    x, y = torch.zeros(32), torch.zeros(32)
    graph = object()
    with rec:
        rec.on(1)
        x.add_(1.0)                           # warm-up on the side stream
        rec.on(7)
        with rec.capture(graph):
            n = len(rec.checker.launches)
            torch.mul(x, 2.0, out=y)          # captured: belongs to the graph, nothing runs
            assert len(rec.checker.launches) == n
        rec.on(0)
        rec.replay(graph)                     # not ordered after the warm-up
        assert [(r.kind, r.second.name) for r in rec.checker.reports] == [("write->read", "graph.replay")]
        rec.checker.wait_stream(0, 1)
        rec.replay(graph)
        assert len(rec.checker.reports) == 1
        rec.on(2)
        y.sum()                               # a reader of the graph's output on another stream
    assert [(r.first.name, r.second.name) for r in rec.checker.reports[1:]] == [("graph.replay", "aten.sum")]


def test_autograd_hand_off_between_streams_is_modelled(rec):
    """the engine runs a node on the stream of its forward op (the stand-in: a pre-hook registered ahead of the recorder's) and orders it
    after the nodes that produced its incoming gradients"""
    w1, w2 = torch.ones(16, requires_grad=True), torch.ones(16, requires_grad=True)
    x = torch.ones(16)
    with rec:
        rec.on(1)
        a = (w1 * x) * 2.0
        a.grad_fn.register_prehook(lambda g: rec.on(1))
        rec.on(2)
        b = (w2 + x) * 3.0
        b.grad_fn.register_prehook(lambda g: rec.on(2))
        rec.checker.wait_stream(0, 1)
        rec.checker.wait_stream(0, 2)
        rec.on(0)
        loss = (a + b).sum()
        assert not rec.checker.reports
        loss.backward()
        # the gradient made on stream 0 is read by the two branches on streams 1 and 2: ordered by the engine's hand-off
        assert not rec.errors and not rec.checker.reports, rec.lines()
        on = {l.stream for l in rec.checker.launches[-6:]}
        assert {1, 2} <= on and rec.checker.ordered >= 4
        # what the engine does NOT order: the caller reading a gradient that a side stream wrote
        rec.on(0)
        w2.grad.sum()
    assert [(r.kind, r.first.stream, r.second.name) for r in rec.checker.reports] == [("write->read", 2, "aten.sum")], rec.lines()


def test_recorder_restores_what_it_shadows():
    before = (torch.cuda.Event.record, torch.cuda.Event.wait, torch.cuda.Event.query, torch.cuda.synchronize, torch.autograd.backward,
              torch.cuda.CUDAGraph.replay)
    with SA.Recorder(stream_of=lambda: 0, all_tensors=True):
        assert torch.cuda.Event.record is not before[0]
    assert before == (torch.cuda.Event.record, torch.cuda.Event.wait, torch.cuda.Event.query, torch.cuda.synchronize, torch.autograd.backward,
                      torch.cuda.CUDAGraph.replay)


def test_stream_primitives_are_written_on_the_shadowed_ones():
    """Stream.wait_stream / wait_event / record_event are Python on top of Event.record / Event.wait in torch: the recorder shadows the
    latter only, so this must stay true"""
    import inspect
    S = torch.cuda.Stream
    assert "wait_event" in inspect.getsource(S.wait_stream) and "record_event" in inspect.getsource(S.wait_stream)
    assert "event.wait(self)" in inspect.getsource(S.wait_event) and "event.record(self)" in inspect.getsource(S.record_event)


# ---- naming ------------------------------------------------------------------------------------------------------------------------------
def test_catalog_names_the_most_specific_attribute():
    class Layer:
        pass
    flat = torch.zeros(128)
    layer, child = Layer(), Layer()
    layer.child = child
    child.kernel = flat[32:64]
    child._folded = ((1, 2), torch.zeros(4), torch.zeros(4))
    child.kernel._shdr_packed = (0, {("x3", 8): (torch.zeros(16), 0, None)})
    slots = {("cpu", 1.0): torch.ones(1)}
    names = SA.catalog({"net": layer, "flat": flat, "_ops._CONST_SLOTS": slots})
    nm = lambda t: SA.name_of(names, *SA.interval(t))      # noqa: E731
    assert nm(child.kernel) == "net.child.kernel" and nm(flat[0:8]) == "flat" and nm(child._folded[2]) == "net.child._folded[2]"
    assert nm(child.kernel._shdr_packed[1][("x3", 8)][0]) == "net.child.kernel._shdr_packed[('x3', 8)]"
    assert nm(slots[("cpu", 1.0)]) == "_ops._CONST_SLOTS[('cpu', 1.0)]"
    assert SA.name_of(names, 1, 2) is None


# ---- the header parser -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def protos():
    return SA.parse_header()


def _rw(params):
    return {p.name: ("r" if p.const else "rw") for p in params if p.pointer and p.name != "stream" and not p.ctype.endswith("desc*")}


def test_parser_constness_of_adam(protos):
    assert _rw(protos["shdr_adam_f32"]) == dict(p="rw", g="r", m="rw", v="rw")
    assert SA.stream_index(protos["shdr_adam_f32"]) == 10


def test_parser_constness_of_the_ranged_convolution(protos):
    ps = protos["shdr_conv2d_fwd_prepared_ranged_f32"]
    assert [p.name for p in ps] == ["d", "x1", "x2", "prepared", "bias", "scale", "shift", "residual", "y", "y_pool", "workspace", "x1_range",
                                    "x2_range", "y_range", "stream"]
    assert _rw(ps) == dict(x1="r", x2="r", prepared="r", bias="r", scale="r", shift="r", residual="r", y="rw", y_pool="rw", workspace="rw",
                           x1_range="r", x2_range="r", y_range="rw")
    assert ps[0].const and ps[0].ctype == "const shdr_conv2d_desc*" and SA.stream_index(ps) == 14


def test_parser_constness_of_absmax(protos):
    ps = protos["shdr_absmax_f32"]
    assert [(p.name, p.pointer, p.const) for p in ps] == [("x", True, True), ("n", False, False), ("out", True, False), ("stream", True, False)] or \
        [(p.pointer, p.const) for p in ps] == [(True, True), (False, False), (True, False), (True, False)]
    assert SA.stream_index(ps) == 3


def test_parser_covers_every_bound_symbol_with_a_stream(protos):
    """every symbol of _lib.SIGNATURES is parsed with the arity ctypes binds, pointers where ctypes has pointers; the ones whose prototype
    ends in `void* stream` are the launches the recorder wraps"""
    import ctypes
    L = importlib.import_module("singlehdr-tf2_amd._lib")
    launches = 0
    for name, (_, argtypes) in L.SIGNATURES.items():
        assert name in protos, name
        ps = protos[name]
        assert len(ps) == len(argtypes), (name, len(ps), len(argtypes))
        for p, a in zip(ps, argtypes):
            is_ptr = a is ctypes.c_void_p or a is ctypes.c_char_p or hasattr(a, "contents") or (isinstance(a, type) and issubclass(a, ctypes._Pointer))
            assert p.pointer == is_ptr, (name, p, a)
        si = SA.stream_index(ps)
        if si is not None:
            launches += 1
            assert si == len(ps) - 1 or ps[si + 1].name in ("stage_ms", "ms"), (name, si)
    assert launches >= 140, launches
