"""The multi-stream and graphed schedules under the happens-before audit (tests/stream_audit.py), and their bits against a one-stream run.

Every case builds fresh models, so every per-version cache (prepared filters, folded BatchNorm, padded and composed filters, the inverse-CRF
table, the constant range slots) is cold, and runs the schedule under one recorder: zero unordered cross-stream conflicting pairs.  The
audit decides ordering on the host, from what was enqueued where: it gives the same answer on every run and does not depend on which
stream happens to run first.  It sees ordering, not arithmetic, so the second half compares bits: slice k of a multi-stream call equals a
one-stream call on exactly that slice (same images, same plans, same ranges: no tolerance)."""
import numpy as np
import pytest
import torch

import stream_audit as SA
from conftest import quantised_image
from oracle import nets
from test_gpu_joint import make_batch

pytestmark = pytest.mark.gpu

MODULES = {"deq": "dequantization_net", "lin": "linearization_net", "hal": "hallucination_net", "ref": "refinement_net"}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def fresh_models(shdr, seed, names=("deq", "lin", "hal", "ref")):
    return {k: getattr(shdr, MODULES[k]).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), seed + i)) for i, k in enumerate(names)}


@pytest.fixture
def cold(shdr, monkeypatch):
    """the module-level cache of constant range slots starts empty, like the per-model caches of fresh models"""
    monkeypatch.setattr(shdr._ops, "_CONST_SLOTS", {})
    torch.cuda.synchronize()
    return shdr._ops


def roots_of(K, models, **more):
    roots = dict(models)
    roots["_ops._CONST_SLOTS"] = K._CONST_SLOTS
    roots.update(more)
    return roots


def finish(rec, roots, label, inference=True):
    """print the counters (pytest -s / -rP shows them), then: launches on at least two streams, for an inference case at least one
    cross-stream pair examined and found ordered, and no report"""
    ck = rec.checker
    print("stream audit [%s]: %s, untracked pointers %d" % (label, ck.summary(), rec.untracked))
    for line in rec.lines(roots):
        print("  " + line)
    assert not rec.errors, rec.errors[0]
    assert len(ck.streams()) >= 2, ck.streams()
    if inference:
        assert ck.examined >= 1 and ck.ordered >= 1, ck.summary()
    rec.assert_clean(roots)


def inference_of(shdr, ms, **kw):
    return shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms.get("ref"), **kw)


# ---- the schedules under the audit ------------------------------------------------------------------------------------------------------
def audit_inference(shdr, K, streams, batch, precision, label):
    ms = fresh_models(shdr, 300)
    run = inference_of(shdr, ms, streams=streams, precision=precision)
    x = dev(quantised_image(np.random.default_rng(40), (batch, 64, 96, 3)))
    torch.cuda.synchronize()
    with SA.Recorder(K) as rec:
        first = run(x)                      # every cache cold: produced on the stream of the slice that asks first
        second = run(x)
    finish(rec, roots_of(K, ms), label)
    assert len(rec.checker.streams()) >= streams
    assert torch.equal(first, second)


def test_inference_two_streams(shdr, cold, split_forced):
    audit_inference(shdr, cold, 2, 4, "fp32", "Inference(streams=2), %s" % ("split_forced" if split_forced else "planned"))


def test_inference_two_streams_fp16(shdr, cold):
    audit_inference(shdr, cold, 2, 4, "fp16", "Inference(streams=2), fp16")


def test_inference_three_streams(shdr, cold):
    audit_inference(shdr, cold, 3, 3, "fp32", "Inference(streams=3)")


def joint_setup(shdr, **kw):
    ms = fresh_models(shdr, 310, ("deq", "lin", "hal"))
    V = nets.init_params(nets.vgg_spec(), 313)
    dd = {n: [V[n + ".kernel"], V[n + ".bias"]] for n in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3")}
    step = shdr.pipeline.JointTrainStep(ms["deq"], ms["lin"], ms["hal"], shdr.vgg16.Vgg16(data_dict=dd), lr=1e-3, **kw)
    batch, inv = make_batch(np.random.default_rng(41), 3, 64)
    return ms, step, tuple(dev(t) for t in batch), dev(inv)


def test_cold_caches_after_a_weight_update(shdr, cold):
    """two multi-stream joint steps, then a two-stream inference on the same models: every version has bumped, every cache is cold again.
    Adam and the next zero_grad on the main stream against the side-stream backward writes into FlatParams.grad, and the BatchNorm
    moving statistics against the next forward, are among the pairs that must come out ordered."""
    K = cold
    ms, step, batch, inv = joint_setup(shdr)
    assert step.multi_stream
    run = inference_of(shdr, ms, streams=2)
    torch.cuda.synchronize()
    with SA.Recorder(K) as rec:
        step(batch, inv, apply=True)
        step(batch, inv, apply=True)
        out = run(batch[0])
    roots = roots_of(K, ms, **{"step.params": step.params})
    finish(rec, roots, "2 x JointTrainStep(multi_stream) + Inference(streams=2)")
    ck = rec.checker
    assert len(ck.streams()) >= 6                                       # main, three training streams, two inference streams
    adam = [l for l in ck.launches if l.name == "shdr_adam_f32"]
    assert len(adam) == 2 and bool(torch.isfinite(out).all())
    # the pairs named above were really examined: the side streams wrote into the flat gradient that Adam reads on another stream
    grad = SA.interval(step.params.grad)
    writers = {l.stream for l in ck.launches if l.stream != adam[0].stream and any(lo < grad[1] and grad[0] < hi for lo, hi in l.writes)}
    assert len(writers) >= 3, writers


def test_graphed_inference(shdr, cold):
    K = cold
    ms = fresh_models(shdr, 320)
    run = shdr.pipeline.GraphedInference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], copy_output=True)
    rng = np.random.default_rng(42)
    x, x2, y = dev(quantised_image(rng, (1, 64, 96, 3))), dev(quantised_image(rng, (1, 64, 96, 3))), dev(quantised_image(rng, (1, 64, 64, 3)))
    torch.cuda.synchronize()
    with SA.Recorder(K) as rec:
        a = run(x)                          # warm-up on the side stream, capture, first replay
        b = run(x2)                         # replay
        c = run(x)                          # replay
        d = run(y)                          # a second input shape: a second warm-up and capture
    finish(rec, roots_of(K, ms), "GraphedInference")
    replays = [l for l in rec.checker.launches if l.name == "graph.replay"]
    assert len(replays) == 4 and len(rec.graphs) == 2 and all(l.reads and l.writes for l in replays)
    assert torch.equal(a, c) and not torch.equal(a, b) and tuple(d.shape) == (1, 64, 64, 3)


# ---- the auditor can fail on the real code ------------------------------------------------------------------------------------------------
def test_missing_wait_in_the_filter_cache_is_reported(shdr, cold, monkeypatch):
    K = cold

    def get_without_wait(w, attr, key):
        store = getattr(w, attr, None)
        if store is None or store[0] != w._version:
            return None
        ent = store[1].get(key)
        return None if ent is None else ent[0]
    monkeypatch.setattr(K, "_filter_cache_get", get_without_wait)
    ms = fresh_models(shdr, 330)
    run = inference_of(shdr, ms, streams=2)
    x = dev(quantised_image(np.random.default_rng(43), (4, 64, 96, 3)))
    torch.cuda.synchronize()
    with SA.Recorder(K) as rec:
        run(x)
    lines = rec.lines(roots_of(K, ms))
    packed = [(r, l) for r, l in zip(rec.checker.reports, lines) if "_shdr_packed" in l]
    assert packed, lines
    r = packed[0][0]
    assert r.kind == "write->read" and "prepare_filter" in r.first.name and r.first.stream != r.second.stream, packed[0][1]


def test_missing_join_in_front_of_the_concatenation_is_reported(shdr, cold, monkeypatch):
    K = cold
    P = shdr.pipeline

    def call_without_join(self, ldr, return_intermediates=False):
        with torch.no_grad(), K.precision(self.precision):
            main = torch.cuda.current_stream()
            outs = []
            for st, part in zip(self._streams, torch.chunk(ldr, len(self._streams), dim=0)):
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    outs.append(self._run(part.contiguous(), False))
            for o in outs:
                o.record_stream(main)
            return torch.cat(outs, dim=0)
    monkeypatch.setattr(P.Inference, "__call__", call_without_join)
    ms = fresh_models(shdr, 340)
    run = inference_of(shdr, ms, streams=2)
    x = dev(quantised_image(np.random.default_rng(44), (4, 64, 96, 3)))
    torch.cuda.synchronize()
    with SA.Recorder(K) as rec:
        run(x)
    torch.cuda.synchronize()
    cat = [r for r in rec.checker.reports if r.second.name == "aten.cat"]
    assert cat and all(r.kind == "write->read" and r.first.stream != r.second.stream for r in cat), rec.lines()


def test_missing_join_in_front_of_adam_is_reported(shdr, cold, monkeypatch):
    K = cold
    monkeypatch.setattr(shdr.pipeline.JointTrainStep, "_join_streams", lambda self: None)
    ms, step, batch, inv = joint_setup(shdr)
    torch.cuda.synchronize()
    with SA.Recorder(K) as rec:
        step(batch, inv, apply=True)
    torch.cuda.synchronize()
    lines = rec.lines(roots_of(K, ms, **{"step.params": step.params}))
    adam = [(r, l) for r, l in zip(rec.checker.reports, lines) if r.second.name == "shdr_adam_f32"]
    assert adam, lines
    grads = [(r, l) for r, l in adam if ".grad" in l]             # (the rest: Adam rewrites variables the side streams still read)
    assert {r.first.stream for r, _ in grads} >= set(s.cuda_stream for s in step._streams), lines
    assert all(r.kind in ("write->read", "write->write") for r, _ in grads), lines


# ---- the bits, schedule against schedule ---------------------------------------------------------------------------------------------------
def assert_slices_equal_one_stream(shdr, ms, x, streams, precision="fp32", calls=3):
    """slice k of Inference(streams=s)(x) is torch.equal to a one-stream Inference on exactly that slice, in each of `calls` calls"""
    one = inference_of(shdr, ms, precision=precision)
    many = inference_of(shdr, ms, streams=streams, precision=precision)
    parts = torch.chunk(x, streams, dim=0)
    want = [one(p.contiguous()).clone() for p in parts]
    torch.cuda.synchronize()
    for call in range(calls):
        got = many(x)
        torch.cuda.synchronize()
        k0 = 0
        for k, w in enumerate(want):
            g = got[k0:k0 + w.shape[0]]
            k0 += w.shape[0]
            assert torch.equal(g, w), "call %d, slice %d of %d: max |diff| %.3g of max %.3g" % (
                call, k, streams, float((g - w).abs().max()), float(w.abs().max()))
        assert k0 == x.shape[0]


def test_two_stream_slices_equal_one_stream_bits(shdr, split_forced):
    ms = fresh_models(shdr, 350)
    assert_slices_equal_one_stream(shdr, ms, dev(quantised_image(np.random.default_rng(45), (4, 64, 96, 3))), 2)


def test_two_stream_slices_equal_one_stream_bits_fp16(shdr):
    ms = fresh_models(shdr, 350)
    assert_slices_equal_one_stream(shdr, ms, dev(quantised_image(np.random.default_rng(45), (4, 64, 96, 3))), 2, precision="fp16")


def test_three_stream_slices_equal_one_stream_bits(shdr):
    ms = fresh_models(shdr, 350)
    assert_slices_equal_one_stream(shdr, ms, dev(quantised_image(np.random.default_rng(46), (3, 64, 96, 3))), 3)


def test_two_stream_slices_equal_one_stream_bits_256(shdr):
    """8 x 256 x 256: the wide 3x3 layers take the split-operand plan unforced, and the two slices' kernels are large enough to overlap"""
    ms = fresh_models(shdr, 360)
    K = shdr._ops
    assert K.conv2d_plan((4, 256, 256, 64), (3, 3, 64, 64)) == "x3"
    assert_slices_equal_one_stream(shdr, ms, dev(quantised_image(np.random.default_rng(47), (8, 256, 256, 3))), 2)
