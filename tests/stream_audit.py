"""Happens-before audit of what the host enqueues on HIP streams -- test infrastructure.

Every kernel of the package is held to a reference per element; what that cannot see is the SCHEDULE: whether work on one stream is ordered
after the work on another stream that produced its operands.  A race of that kind cannot be exposed by timing on a shared machine, but it
can be decided on the host: record what was enqueued where, with the bytes it reads and writes, record every ordering primitive, and
check the happens-before relation with vector clocks.  That is deterministic and needs no large shapes.

  parse_header(path)        {entry point: [Param]} from the prototypes of include/shdr.h: which pointer is `const` (read) and which is not
                            (read and written), and which argument is the stream.  No hand-written table.
  Checker                   vector clocks per stream and one for the host; per byte interval the last write and the reads since; every
                            conflicting pair on different streams that is not ordered becomes a Report.  Fed by the recorder or by hand.
  Recorder(K)               context manager.  Shadows K._ptr (pointer -> tensor at the call site) and K._lib.load (every C ABI launch:
                            name, stream, device-pointer arguments as byte intervals), runs a TorchDispatchMode (every aten op on
                            torch.cuda.current_stream()), and shadows the ordering primitives of torch.cuda (Event.record / wait / query /
                            synchronize, Stream.synchronize, torch.cuda.synchronize -- Stream.wait_stream, wait_event and record_event are
                            written on top of those), CUDAGraph capture / replay and torch.autograd.backward (the engine's own
                            producer -> consumer stream hand-off between backward nodes, which happens below Python).
  catalog(roots) / name_of  a byte interval -> the attribute of a model, layer, variable or `_ops` global that holds it

The recorder adds no synchronisation and no device work: every shadow calls the original first and then writes a log entry.
What the audit cannot see: races INSIDE a kernel, collectives (RCCL orders its own streams), host threads that enqueue concurrently, a
device pointer handed over as a bare integer (counted in `untracked`), and orderings made below Python other than the autograd hand-off
(they would show as false reports, never as a missed one).  Importing this module needs no GPU.
"""
import bisect
import collections
import contextlib
import ctypes
import os
import re

import torch
from torch.utils._python_dispatch import TorchDispatchMode

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "shdr.h")

# ---- the prototypes -----------------------------------------------------------------------------------------------------------------
Param = collections.namedtuple("Param", "name ctype pointer const")


def parse_header(path=HEADER):
    """{name: [Param]} of every `shdr_*` prototype.  pointer: the declarator has a `*`; const: `const` stands in front of it (the pointee
    is read only)."""
    with open(path) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    protos = {}
    for m in re.finditer(r"\b(shdr_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        name, inner = m.group(1), " ".join(m.group(2).split())
        params = []
        if inner and inner != "void":
            for p in inner.split(","):
                p = p.strip()
                ident = re.search(r"(\w+)\s*(\[\s*\w*\s*\])?$", p)
                ctype = p[:ident.start()].strip()
                pointer = "*" in ctype or ident.group(2) is not None
                params.append(Param(ident.group(1), ctype, pointer, pointer and bool(re.match(r"const\b", ctype))))
        protos[name] = params
    return protos


def stream_index(params):
    """position of the `void* stream` argument, or None"""
    for i, p in enumerate(params):
        if p.name == "stream" and p.pointer and p.ctype.replace(" ", "") == "void*":
            return i
    return None


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
class Launch:
    """one enqueued piece of device work: idx (position in the log), name (entry point or aten op), stream, epoch (its count on that
    stream), reads / writes [(lo, hi)] byte intervals"""
    __slots__ = ("idx", "name", "stream", "epoch", "reads", "writes")

    def __init__(self, idx, name, stream, epoch, reads, writes):
        self.idx, self.name, self.stream, self.epoch, self.reads, self.writes = idx, name, stream, epoch, reads, writes

    def __repr__(self):
        return "#%d %s on stream %s" % (self.idx, self.name, _sname(self.stream))


def _sname(s):
    return "0x%x" % s if isinstance(s, int) and s > 0xffff else str(s)


class Report:
    """an unordered conflicting pair: kind ("write->read" | "read->write" | "write->write"), first / second (Launch), lo / hi (the first
    overlapping bytes found)"""

    def __init__(self, kind, first, second, lo, hi):
        self.kind, self.first, self.second, self.lo, self.hi = kind, first, second, lo, hi

    def line(self, names=None):
        where = "bytes [0x%x, 0x%x)" % (self.lo, self.hi)
        if names is not None:
            n = name_of(names, self.lo, self.hi)
            where = "%s %s" % (n or "<unnamed tensor>", where)
        return "%s not ordered: %r, then %r: %s" % (self.kind, self.first, self.second, where)

    __repr__ = line


class _Seg:
    __slots__ = ("lo", "hi", "w", "r")

    def __init__(self, lo, hi, w=None, r=None):
        self.lo, self.hi, self.w, self.r = lo, hi, w, {} if r is None else r


class Checker:
    """Vector clocks: clock[s][t] = the epoch of stream t up to which t's work is ordered before what s runs next; the host's clock holds
    what is known complete and is joined into a stream's clock with everything enqueued on it.  The byte map is a sorted list of disjoint
    segments, each with its last write and, per stream, the latest read since.
    Counters: launches, examined (cross-stream conflicting pairs), ordered, and reports (a list)."""

    def __init__(self):
        self.clock = {}
        self.host = {}
        self.events = {}
        self.launches = []
        self.log = []
        self.reports = []
        self.examined = self.ordered = 0
        self._starts, self._segs = [], []

    # -- clocks
    def _clk(self, s):
        c = self.clock.get(s)
        if c is None:
            c = self.clock[s] = {}
        return c

    @staticmethod
    def _join(into, other):
        for k, v in other.items():
            if into.get(k, 0) < v:
                into[k] = v

    def _enqueue(self, s):
        c = self._clk(s)
        self._join(c, self.host)
        return c

    # -- ordering primitives
    def record(self, event, stream):
        self.log.append(("record", event, stream))
        self.events[event] = dict(self._enqueue(stream))

    def wait_event(self, stream, event):
        self.log.append(("wait_event", stream, event))
        self._join(self._enqueue(stream), self.events.get(event, {}))

    def wait_stream(self, waiter, waited):
        self.log.append(("wait_stream", waiter, waited))
        self._join(self._enqueue(waiter), self._enqueue(waited))

    def query_true(self, event):
        """the event answered a query with True: what it covers is complete"""
        self.log.append(("query_true", event))
        self._join(self.host, self.events.get(event, {}))

    def sync_event(self, event):
        self.log.append(("sync_event", event))
        self._join(self.host, self.events.get(event, {}))

    def sync_stream(self, stream):
        """the host waited for the stream (Stream.synchronize, a device-to-host read on it)"""
        self.log.append(("sync_stream", stream))
        self._join(self.host, self._enqueue(stream))

    def sync_all(self):
        self.log.append(("sync_all",))
        for s in list(self.clock):
            self._join(self.host, self._enqueue(s))

    # -- launches
    def launch(self, name, stream, reads=(), writes=()):
        """enqueue one piece of work; returns its Launch.  reads / writes: [(lo, hi)] byte intervals (hi exclusive)"""
        c = self._enqueue(stream)
        epoch = c.get(stream, 0) + 1
        c[stream] = epoch
        l = Launch(len(self.log), name, stream, epoch, [iv for iv in reads if iv[1] > iv[0]], [iv for iv in writes if iv[1] > iv[0]])
        self.log.append(("launch", l))
        self.launches.append(l)
        seen = set()
        for lo, hi in l.reads:
            for seg in self._cover(lo, hi):
                if seg.w is not None:
                    self._pair("write->read", seg.w, l, seg, seen)
        for lo, hi in l.writes:
            for seg in self._cover(lo, hi):
                if seg.w is not None:
                    self._pair("write->write", seg.w, l, seg, seen)
                for r in seg.r.values():
                    self._pair("read->write", r, l, seg, seen)
        # (state after the checks: a launch that reads and writes the same bytes does not conflict with itself)
        for lo, hi in l.reads:
            for seg in self._cover(lo, hi):
                seg.r[stream] = l
        for lo, hi in l.writes:
            for seg in self._cover(lo, hi):
                seg.w, seg.r = l, {}
        return l

    def _pair(self, kind, first, second, seg, seen):
        if first.stream == second.stream or first is second or (kind, first.idx) in seen:
            return
        seen.add((kind, first.idx))
        self.examined += 1
        if self.clock[second.stream].get(first.stream, 0) >= first.epoch:
            self.ordered += 1
        else:
            self.reports.append(Report(kind, first, second, seg.lo, seg.hi))

    def _cover(self, lo, hi):
        """the segments that tile [lo, hi) exactly: existing ones are split at lo and hi, gaps are filled"""
        starts, segs = self._starts, self._segs
        i = bisect.bisect_right(starts, lo) - 1
        if i >= 0 and segs[i].hi > lo:
            if segs[i].lo < lo:                       # split at lo
                s = segs[i]
                right = _Seg(lo, s.hi, s.w, dict(s.r))
                s.hi = lo
                i += 1
                starts.insert(i, lo)
                segs.insert(i, right)
        else:
            i += 1
        out, pos = [], lo
        while pos < hi:
            if i < len(segs) and segs[i].lo == pos:
                s = segs[i]
                if s.hi > hi:                         # split at hi
                    right = _Seg(hi, s.hi, s.w, dict(s.r))
                    s.hi = hi
                    starts.insert(i + 1, hi)
                    segs.insert(i + 1, right)
            else:
                end = min(hi, segs[i].lo) if i < len(segs) else hi
                s = _Seg(pos, end)
                starts.insert(i, pos)
                segs.insert(i, s)
            out.append(s)
            pos = s.hi
            i += 1
        return out

    # -- results
    def streams(self):
        return {l.stream for l in self.launches}

    def summary(self):
        return "launches %d on %d stream(s), cross-stream conflicting pairs %d, ordered %d, reports %d" % (
            len(self.launches), len(self.streams()), self.examined, self.ordered, len(self.reports))

    def run(self, log):
        """feed a hand-written log: ("launch", name, stream, reads, writes) or (primitive, *arguments)"""
        for entry in log:
            getattr(self, entry[0])(*entry[1:])
        return self


# ---- naming ------------------------------------------------------------------------------------------------------------------------------
def interval(t):
    """(lo, hi) of the bytes a tensor can touch: data_ptr() and the span of its strides, not its whole storage"""
    if t.numel() == 0:
        return (0, 0)
    span = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))
    lo = t.data_ptr()
    return (lo, lo + span * t.element_size())


FILTER_CACHES = ("_shdr_packed", "_shdr_packed_h", "_shdr_wino")


def catalog(roots, depth=6):
    """[(lo, hi, name)] of every tensor reachable from `roots` {prefix: object}: attributes of layers (children, variables, per-version
    caches held as tuples / dicts), the derived forms kept ON a filter tensor (_ops._filter_cache_put), module globals that are dicts of
    tensors (_ops._CONST_SLOTS)"""
    out, seen = [], set()

    def visit(obj, name, d):
        if obj is None or d < 0 or isinstance(obj, (str, bytes, int, float, bool)):
            return
        if isinstance(obj, torch.Tensor):
            if (id(obj), name) in seen:
                return
            seen.add((id(obj), name))
            lo, hi = interval(obj)
            if hi > lo:
                out.append((lo, hi, name))
            if obj.grad is not None and obj.is_leaf:
                visit(obj.grad, name + ".grad", 0)
            for attr in FILTER_CACHES:
                store = getattr(obj, attr, None)
                if isinstance(store, tuple) and len(store) == 2 and isinstance(store[1], dict):
                    for key, ent in store[1].items():
                        visit(ent[0] if isinstance(ent, tuple) else ent, "%s.%s[%r]" % (name, attr, key), 0)
            return
        if id(obj) in seen:
            return
        seen.add(id(obj))
        if isinstance(obj, dict):
            for k, v in obj.items():
                visit(v, "%s[%r]" % (name, k), d - 1)
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                visit(v, "%s[%d]" % (name, i), d - 1)
        elif hasattr(obj, "__dict__") and not isinstance(obj, type) and type(obj).__module__ not in ("builtins", "torch"):
            for k, v in list(vars(obj).items()):
                if k in ("_children", "_vars"):
                    continue
                visit(v, "%s.%s" % (name, k), d - 1)
    for prefix, root in roots.items():
        visit(root, prefix, depth)
    return out


def name_of(names, lo, hi):
    """the most specific catalogued tensor that overlaps [lo, hi)"""
    best = None
    for a, b, n in names:
        if a < hi and lo < b and (best is None or b - a < best[0]):
            best = (b - a, n)
    return None if best is None else best[1]


# ---- the recorder ------------------------------------------------------------------------------------------------------------------------
class _TPtr(ctypes.c_void_p):
    """what the shadowed K._ptr returns: the c_void_p the library takes, with the byte interval and shape of the tensor it points into"""
    interval = None
    what = None


NO_DEVICE_WORK = ("empty", "new_empty", "empty_like", "empty_strided", "new_empty_strided", "record_stream", "_has_compatible_shallow_copy_type",
                  "is_pinned", "sym_size", "sym_stride", "sym_numel", "sym_storage_offset", "alias", "lift_fresh", "_pin_memory", "set_")
HOST_SCALAR = ("_local_scalar_dense", "item", "equal", "is_nonzero", "allclose")


def _flat_tensors(x, out):
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _flat_tensors(v, out)
    elif isinstance(x, dict):
        for v in x.values():
            _flat_tensors(v, out)
    return out


def _storage(t):
    try:
        return t.untyped_storage().data_ptr()
    except Exception:
        return None


class Recorder(TorchDispatchMode):
    """with Recorder(K) as rec: <the schedule>; then rec.checker.reports, rec.lines(roots), rec.checker.summary().
    K: the `_ops` module whose launches are recorded (None: aten ops and primitives only).
    stream_of: () -> the id of the current stream (default: torch.cuda.current_stream().cuda_stream); all_tensors: count CPU tensors as
    device memory -- both for driving the aten recorder without a GPU."""

    def __init__(self, K=None, stream_of=None, all_tensors=False):
        super().__init__()
        self.K, self.all_tensors = K, all_tensors
        self.stream_of = stream_of if stream_of is not None else (lambda: torch.cuda.current_stream().cuda_stream)
        self.checker = Checker()
        self.protos = parse_header() if K is not None else {}
        self.untracked = 0                  # device-looking pointer arguments that did not come through K._ptr
        self.graphs = {}                    # id(graph) -> (graph, reads, writes): what a capture read and wrote
        self._graph = None                  # the open capture (between CUDAGraph.capture_begin and capture_end, both shadowed: the
                                            # interval in which torch.cuda.is_current_stream_capturing() holds)
        self._saved, self._keep, self.errors = [], [], []

    # -- plumbing
    def _patch(self, obj, name, new):
        self._saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, new)

    def _is_dev(self, t):
        return self.all_tensors or t.is_cuda

    @contextlib.contextmanager
    def capture(self, graph):
        """stand-in for a stream capture (without a GPU): launches inside belong to `graph`"""
        self._begin_capture(graph)
        try:
            yield
        finally:
            self._graph = None

    def _begin_capture(self, graph):
        self._graph = self.graphs.setdefault(id(graph), (graph, [], []))

    def replay(self, graph, stream=None):
        """one launch on the replaying stream that reads and writes everything the capture read and wrote"""
        _, reads, writes = self.graphs[id(graph)]
        return self.checker.launch("graph.replay", self.stream_of() if stream is None else stream, reads, writes)

    def _launch(self, name, stream, reads, writes):
        if self._graph is not None:
            self._graph[1].extend(reads)
            self._graph[2].extend(writes)
            return None
        return self.checker.launch(name, stream, reads, writes)

    # -- C ABI launches
    def _wrap_entry(self, name, fn, params, si):
        def launch(*args):
            rc = fn(*args)
            reads, writes = [], []
            for p, a in zip(params, args):
                if isinstance(a, _TPtr):
                    reads.append(a.interval)
                    if not p.const:
                        writes.append(a.interval)
                elif p.pointer and p.name != "stream" and not p.ctype.startswith(("shdr_", "const shdr_")) \
                        and isinstance(a, (int, ctypes.c_void_p)) and getattr(a, "value", a):
                    self.untracked += 1              # a pointer that did not come through K._ptr (a bare integer, a host buffer)
            s = args[si]
            s = getattr(s, "value", s) or 0
            self._launch(name, s, reads, writes)
            return rc
        launch.__name__ = name
        return launch

    def _install_abi(self):
        K, rec = self.K, self
        lib_mod = K._lib
        real = lib_mod.load()

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                params = rec.protos.get(name)
                si = None if params is None else stream_index(params)
                if si is None:
                    return fn
                w = rec._wrap_entry(name, fn, params, si)
                object.__setattr__(self, name, w)
                return w
        proxy = Proxy()
        self._patch(lib_mod, "load", lambda: proxy)

        def ptr(t):
            if t is None:
                return None
            p = _TPtr(t.data_ptr())
            p.interval, p.what = interval(t), (tuple(t.shape), t.dtype)
            return p
        self._patch(K, "_ptr", ptr)

    # -- aten ops
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        try:
            self._aten(func, args, kwargs, out)
        except Exception as e:               # the audit must never change what runs: a recording error is kept, not raised
            self.errors.append(e)
        return out

    def _aten(self, func, args, kwargs, out):
        name = func._schema.name.split("::")[-1]
        if name in NO_DEVICE_WORK:
            return
        ins = [t for t in _flat_tensors((args, kwargs), []) if self._is_dev(t)]
        outs_all = _flat_tensors(out, [])
        outs = [t for t in outs_all if self._is_dev(t)]
        if not ins and not outs:
            return
        written_all = []
        for i, sa in enumerate(func._schema.arguments):
            if sa.alias_info is not None and sa.alias_info.is_write:
                _flat_tensors(args[i] if i < len(args) else kwargs.get(sa.name), written_all)
        written = [t for t in written_all if self._is_dev(t)]
        in_storages = {_storage(t) for t in ins}
        written_ids = {id(t) for t in written}
        fresh = [t for t in outs if _storage(t) not in in_storages and id(t) not in written_ids]
        # a device-to-host read makes the host wait for the stream it runs on (unless it was asked not to block)
        to_host = not self.all_tensors and any(not t.is_cuda for t in outs_all + written_all)
        non_blocking = bool(kwargs.get("non_blocking")) or (name == "copy_" and len(args) > 2 and bool(args[2]))
        host_read = bool(ins) and (name in HOST_SCALAR or (to_host and not non_blocking))
        if not written and not fresh and not host_read:
            return                               # a view: the returns alias an input and nothing is written
        s = self.stream_of()
        self._launch("aten." + name, s, [interval(t) for t in ins], [interval(t) for t in written + fresh])
        if host_read and self._graph is None:
            self.checker.sync_stream(s)

    # -- ordering primitives of torch.cuda, graphs, the autograd engine
    def _install_cuda(self):
        ck, rec = self.checker, self
        Event, Stream = torch.cuda.Event, torch.cuda.Stream
        sid = lambda st: rec.stream_of() if st is None else st.cuda_stream      # noqa: E731

        def shadow(cls, name, after):
            orig = getattr(cls, name)

            def shadowed(self, *a, **kw):
                res = orig(self, *a, **kw)
                after(self, res, *a, **kw)
                return res
            shadowed.__name__ = name
            rec._patch(cls, name, shadowed)

        def ev(e):
            rec._keep.append(e)                  # (an id is reused once its object dies)
            return id(e)
        shadow(Event, "record", lambda e, res, stream=None: ck.record(ev(e), sid(stream)))
        shadow(Event, "wait", lambda e, res, stream=None: ck.wait_event(sid(stream), id(e)))
        shadow(Event, "query", lambda e, res: ck.query_true(id(e)) if res else None)
        shadow(Event, "synchronize", lambda e, res: ck.sync_event(id(e)))
        shadow(Stream, "synchronize", lambda st, res: ck.sync_stream(st.cuda_stream))
        orig_sync = torch.cuda.synchronize

        def synchronize(*a, **kw):
            res = orig_sync(*a, **kw)
            ck.sync_all()
            return res
        self._patch(torch.cuda, "synchronize", synchronize)
        G = torch.cuda.CUDAGraph
        shadow(G, "capture_begin", lambda g, res, *a, **kw: rec._begin_capture(g))
        shadow(G, "capture_end", lambda g, res: setattr(rec, "_graph", None))
        shadow(G, "replay", lambda g, res: rec.replay(g))

    def _install_autograd(self):
        """The engine runs a backward node on the stream of its forward op and makes that stream wait for the streams of the nodes that
        produced its incoming gradients (and for the caller's stream at the root).  That happens below Python, so it is restated with
        hooks: a node's post-hook records a stand-in event on the node's stream, the pre-hook of each node it feeds waits for it."""
        ck, rec = self.checker, self
        orig = torch.autograd.backward

        def backward(tensors, *a, **kw):
            roots = [t.grad_fn for t in ([tensors] if isinstance(tensors, torch.Tensor) else list(tensors)) if t.grad_fn is not None]
            producers, nodes, stack, handles = collections.defaultdict(list), {}, list(roots), []
            while stack:
                n = stack.pop()
                if id(n) in nodes:
                    continue
                nodes[id(n)] = n
                for nxt, _ in n.next_functions:
                    if nxt is not None:
                        producers[id(nxt)].append(id(n))
                        stack.append(nxt)
            caller = rec.stream_of()             # (the root's gradients are made on the caller's stream, inside the call below)
            root_ids = {id(n) for n in roots}

            def pre(n):
                def hook(grad_outputs):
                    s = rec.stream_of()
                    if id(n) in root_ids and s != caller:
                        ck.wait_stream(s, caller)
                    for p in producers.get(id(n), ()):
                        if ("node", p) in ck.events:
                            ck.wait_event(s, ("node", p))
                return hook

            def post(n):
                def hook(grad_inputs, grad_outputs):
                    ck.record(("node", id(n)), rec.stream_of())
                return hook
            try:
                for n in nodes.values():
                    handles.append(n.register_prehook(pre(n)))
                    handles.append(n.register_hook(post(n)))
                return orig(tensors, *a, **kw)
            finally:
                for h in handles:
                    h.remove()
                for p in nodes:
                    ck.events.pop(("node", p), None)
        self._patch(torch.autograd, "backward", backward)

    # -- context
    def __enter__(self):
        try:
            if self.K is not None:
                self._install_abi()
            self._install_cuda()
            self._install_autograd()
        except Exception:
            self._restore()
            raise
        return super().__enter__()

    def __exit__(self, *exc):
        try:
            return super().__exit__(*exc)
        finally:
            self._restore()

    def _restore(self):
        for obj, name, old in reversed(self._saved):
            setattr(obj, name, old)
        self._saved = []

    # -- results
    def lines(self, roots=None):
        names = None if roots is None else catalog(roots)
        return [r.line(names) for r in self.checker.reports]

    def assert_clean(self, roots=None):
        assert not self.errors, "the recorder failed on %d op(s): %r" % (len(self.errors), self.errors[0])
        if self.checker.reports:
            raise AssertionError("stream audit: %s\n%s" % (self.checker.summary(), "\n".join(self.lines(roots))))
