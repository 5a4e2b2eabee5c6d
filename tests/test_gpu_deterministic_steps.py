"""The deterministic mode on whole training steps (DESIGN.md section 4 "Deterministic mode"): JointTrainStep, TrainStep("deq" | "lin" | "hal")
and FinetuneStep(precision="fp32") built with deterministic=True.

The set-ups are those of tests/test_gpu_tape_replay.py (imported: the same seeds and shapes -- joint 3 x 64^2, per-network 2 x 64^2,
fine-tuning 2 x 64^2).

  * Reproducible: two freshly built steps from the same seeds, three iterations with apply=True; the losses, the flat gradient, the
    BatchNorm moving statistics and the parameters after Adam are torch.equal at every iteration.  The joint step with multi_stream True and
    False, and the two settings against each other.
  * Counter: K.order_dependent_launches() does not move over a deterministic step and moves over a default one.
  * Still right: every step recorded in deterministic mode with tests/tape_replay.py; every node and every variable on the op-level bars
    (the stem bias of the Linearization-Net as in test_gpu_tape_replay.py: on the fp32 summation bound).
  * One stream per gradient range: the folds write `out = out + S` without an atomic, so no two streams may accumulate into one range of
    the flat gradient: every call that accumulates is logged with its stream in a multi-stream joint step.
  * Refusal (fp16 + deterministic) and scoping (K.DETERMINISTIC after the call is what it was).
"""
import numpy as np
import pytest
import torch

import test_gpu_tape_replay as T
from conftest import quantised_image
from oracle import nets

pytestmark = pytest.mark.gpu

ITERS = 3


def moving_stats(models):
    return [t for m in models for _, t, trainable in m.named_weights() if not trainable]


def state(step, models, losses):
    torch.cuda.synchronize()
    return dict(losses=[t.detach().clone() for t in losses], grad=step.params.grad.clone(), flat=step.params.flat.clone(),
                moving=[t.detach().clone() for t in moving_stats(models)])


def assert_same_state(a, b, what):
    for key in ("losses", "moving"):
        assert len(a[key]) == len(b[key]) and (len(a[key]) > 0 or key == "moving"), (what, key)      # (the Dequantization-Net has no BatchNorm)
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert torch.equal(x, y), "%s: %s[%d] differs (max |d| = %g)" % (what, key, i, float((x - y).abs().max()))
    for key in ("grad", "flat"):
        if not torch.equal(a[key], b[key]):
            i = int(torch.nonzero(a[key] != b[key])[0])
            raise AssertionError("%s: %s differs in %d of %d elements, first at %d: %r vs %r" % (
                what, key, int((a[key] != b[key]).sum()), a[key].numel(), i, float(a[key][i]), float(b[key][i])))


# ---- the steps, built fresh from the seeds of test_gpu_tape_replay.py ------------------------------------------------------------------
def joint_run(shdr, multi_stream, deterministic=True, iters=ITERS):
    rng = np.random.default_rng(11)
    ms, vgg = T.three_nets(shdr, 70)
    batch, inv = T.make_batch(rng, 3, 64)
    step = shdr.pipeline.JointTrainStep(ms["deq"], ms["lin"], ms["hal"], vgg, lr=1e-3, multi_stream=multi_stream, deterministic=deterministic)
    batch, inv = tuple(T.dev(t) for t in batch), T.dev(inv)
    states = []
    for _ in range(iters):
        out = step(batch, inv, apply=True)
        states.append(state(step, list(ms.values()), [out["total"], out["loss_deq"], out["loss_lin"], out["loss_hal"], out["crf_loss"]]))
    return step, ms, states


def per_net_run(shdr, which, deterministic=True, iters=ITERS):
    rng = np.random.default_rng(21)
    ms, vgg = T.three_nets(shdr, 80)
    batch, inv = T.make_batch(rng, 2, 64)
    ldr, jpeg, clipped, hdr_t, mask = (T.dev(t) for t in batch)
    step = shdr.pipeline.TrainStep(which, ms[which], vgg if which == "hal" else None, deterministic=deterministic)
    ds = {"deq": (ldr, jpeg, mask), "lin": (ldr, clipped, mask, T.dev(inv)), "hal": (hdr_t, clipped, mask)}[which]
    states = []
    for _ in range(iters):
        step(ds, apply=True)
        states.append(state(step, [ms[which]], [step.last_loss]))
    return step, ms, ds, states


FT_MODS = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")


def finetune_setup(shdr, **kw):
    rng = np.random.default_rng(12)
    P = {k: nets.init_params(getattr(nets, k + "_spec")(), 95 + i) for i, k in enumerate(FT_MODS)}
    ldr = quantised_image(rng, (2, 64, 64, 3))
    ldr[0, :12, :12] = 1.0
    hdr = rng.random((2, 64, 64, 3)) * 1.5
    hdr = hdr / (1e-6 + hdr.mean(axis=(1, 2, 3), keepdims=True)) * 0.5
    ms = {k: getattr(shdr, FT_MODS[k]).model().load_numpy(P[k]) for k in FT_MODS}
    step = shdr.pipeline.FinetuneStep(ms["deq"], ms["lin"], ms["hal"], ms["ref"], lr=1e-4, **kw)
    return step, ms, T.dev(ldr), T.dev(hdr)


def finetune_run(shdr, deterministic=True, iters=ITERS):
    step, ms, ldr, hdr = finetune_setup(shdr, deterministic=deterministic)
    states = []
    for _ in range(iters):
        out = step(ldr, hdr, apply=True)
        states.append(state(step, list(ms.values()), [out["loss_sum"], out["refinement_output"]]))
    return step, ms, states


# ---- reproducible ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joint_states(shdr):
    """two fresh runs per multi_stream setting"""
    return {ms: [joint_run(shdr, ms)[2] for _ in range(2)] for ms in (True, False)}


@pytest.mark.parametrize("multi_stream", [True, False], ids=["multi_stream", "one_stream"])
def test_joint_step_is_reproducible(joint_states, multi_stream):
    a, b = joint_states[multi_stream]
    for it in range(ITERS):
        assert_same_state(a[it], b[it], "joint step, multi_stream=%s, iteration %d" % (multi_stream, it))
    assert not torch.equal(a[0]["flat"], a[ITERS - 1]["flat"])                      # Adam moved the parameters


def test_joint_step_multi_stream_equals_one_stream(joint_states):
    """the schedule changes which stream a kernel runs on, never what it computes"""
    for it in range(ITERS):
        assert_same_state(joint_states[True][0][it], joint_states[False][0][it], "joint step, multi_stream True vs False, iteration %d" % it)


@pytest.mark.parametrize("which", ["deq", "lin", "hal"])
def test_per_network_step_is_reproducible(shdr, which):
    a, b = per_net_run(shdr, which)[3], per_net_run(shdr, which)[3]
    for it in range(ITERS):
        assert_same_state(a[it], b[it], "TrainStep(%r), iteration %d" % (which, it))
    assert not torch.equal(a[0]["flat"], a[ITERS - 1]["flat"])


def test_finetune_step_is_reproducible(shdr):
    a, b = finetune_run(shdr)[2], finetune_run(shdr)[2]
    for it in range(ITERS):
        assert_same_state(a[it], b[it], "FinetuneStep(fp32), iteration %d" % it)
    assert not torch.equal(a[0]["flat"], a[ITERS - 1]["flat"])


# ---- the counter ------------------------------------------------------------------------------------------------------------------------------
def counted(K, fn):
    before = K.order_dependent_launches()
    fn()
    torch.cuda.synchronize()
    return K.order_dependent_launches() - before


@pytest.mark.parametrize("kind", ["joint_multi_stream", "joint_one_stream", "deq", "lin", "hal", "finetune"])
def test_counter_stands_still_in_deterministic_mode_and_moves_in_default_mode(shdr, kind):
    K = shdr._ops

    def run(deterministic):
        if kind.startswith("joint"):
            return lambda: joint_run(shdr, kind == "joint_multi_stream", deterministic, iters=1)
        if kind == "finetune":
            return lambda: finetune_run(shdr, deterministic, iters=1)
        return lambda: per_net_run(shdr, kind, deterministic, iters=1)
    moved = counted(K, run(False))
    assert moved > 0, "the default step did not move the counter: it is not wired"
    still = counted(K, run(True))
    print("%s: %d order-dependent launches in the default step, %d in the deterministic one" % (kind, moved, still))
    assert still == 0, "%d launches of the deterministic step still depend on the order of atomics" % still


# ---- still right: the deterministic steps on the op-level bars ---------------------------------------------------------------------------
def test_joint_step_tape_in_deterministic_mode(shdr):
    rng = np.random.default_rng(11)
    ms, vgg = T.three_nets(shdr, 70)
    batch, inv = T.make_batch(rng, 3, 64)
    step = shdr.pipeline.JointTrainStep(ms["deq"], ms["lin"], ms["hal"], vgg, lr=1e-3, deterministic=True)
    batch, inv = tuple(T.dev(t) for t in batch), T.dev(inv)
    variables = [v for k in ("deq", "lin", "hal") for v in T.named(k + ".", ms[k])]
    K = shdr._ops
    before = K.order_dependent_launches()
    rec, rep, _ = T.recorded(shdr, lambda: step(batch, inv, apply=False), variables, fanouts=[T.INVCRF_FANOUT])
    assert K.order_dependent_launches() == before
    rep.assert_ok()
    assert {"BlendConstFn", "LogcFn", "TvLossFn", "ApplyRfFn", "ForkFn", "DiffLossFn"} <= T.classes(rec)


@pytest.mark.parametrize("which", ["deq", "lin", "hal"])
def test_per_network_step_tapes_in_deterministic_mode(shdr, which):
    rng = np.random.default_rng(21)
    ms, vgg = T.three_nets(shdr, 80)
    batch, inv = T.make_batch(rng, 2, 64)
    ldr, jpeg, clipped, hdr_t, mask = (T.dev(t) for t in batch)
    step = shdr.pipeline.TrainStep(which, ms[which], vgg if which == "hal" else None, deterministic=True)
    ds = {"deq": (ldr, jpeg, mask), "lin": (ldr, clipped, mask, T.dev(inv)), "hal": (hdr_t, clipped, mask)}[which]
    fan = {"deq": [], "lin": [T.INVCRF_FANOUT], "hal": [T.HAL_LOSS_FANOUT]}[which]
    rec, rep, _ = T.recorded(shdr, lambda: step(ds, apply=False), T.named("", ms[which]), fanouts=fan)
    rep.assert_ok(leave=T.is_stem_bias if which == "lin" else None)
    if which == "lin":                     # the stem bias as in test_linearization_stem_bias_gradient_on_the_model_wide_scale
        T.stem_bias_figures(rec, rep)
        bad = [e for e in rep.entries + rep.var_entries if T.is_stem_bias(e) and not e.ok]
        assert not bad, "\n".join(e.line() for e in bad)


def test_finetune_step_tape_in_deterministic_mode(shdr):
    step, ms, ldr, hdr = finetune_setup(shdr, deterministic=True)
    variables = [v for k in FT_MODS for v in T.named(k + ".", ms[k])]
    rec, rep, _ = T.recorded(shdr, lambda: step(ldr, hdr, apply=False), variables, fanouts=[T.REF_INPUT_FANOUT])
    rep.assert_ok()
    assert {"LinFrontendFn", "AlphaBlendFn", "Pack3Fn", "Unpack3Fn", "MeanNormFn", "ApplyRfFn", "ForkFn"} <= T.classes(rec)


# ---- two streams, one buffer ------------------------------------------------------------------------------------------------------------------
def test_every_gradient_range_is_accumulated_from_one_stream(shdr, monkeypatch):
    """The deterministic folds write out = out + S without an atomic.  In the multi-stream joint step every call that accumulates into the
    flat gradient is logged with its stream: a net's range is written from one stream only, and the three nets' ranges are disjoint."""
    K = shdr._ops
    rng = np.random.default_rng(11)
    ms, vgg = T.three_nets(shdr, 70)
    batch, inv = T.make_batch(rng, 3, 64)
    step = shdr.pipeline.JointTrainStep(ms["deq"], ms["lin"], ms["hal"], vgg, lr=1e-3, multi_stream=True, deterministic=True)
    slices = step._net_slices()
    base, esz = step.params.grad.data_ptr(), step.params.grad.element_size()
    writers = {}                                                   # net -> {stream}

    def log(t):
        if t is None:
            return
        off = (t.data_ptr() - base) // esz
        if 0 <= off < step.params.numel:
            (net,) = [k for k, (b, e) in slices.items() if b <= off and off + t.numel() <= e]
            writers.setdefault(net, set()).add(torch.cuda.current_stream().cuda_stream)

    def wrap(name, outs):
        orig = getattr(K, name)

        def f(*a, **kw):
            assert K.DETERMINISTIC
            for key in outs:
                log(kw.get(key) if isinstance(key, str) else (a[key] if len(a) > key else None))
            return orig(*a, **kw)
        monkeypatch.setattr(K, name, f)
    wrap("conv2d_wgrad", ["out"])
    wrap("bias_grad", ["out"])
    wrap("act_bwd_bias", ["out"])
    wrap("bn_bwd", ["dgamma_out", "dbeta_out", 7, 8])               # (_autograd passes the two buffers by position)
    step(tuple(T.dev(t) for t in batch), T.dev(inv), apply=False)
    torch.cuda.synchronize()
    assert set(writers) == {"deq", "lin", "hal"}, writers
    assert all(len(s) == 1 for s in writers.values()), writers
    assert len({next(iter(s)) for s in writers.values()}) == 3, writers            # three nets, three streams
    bounds = sorted(slices.values())
    assert all(a[1] <= b[0] for a, b in zip(bounds, bounds[1:]))


# ---- refusal and scoping ----------------------------------------------------------------------------------------------------------------------
def test_fp16_with_deterministic_is_refused(shdr):
    with pytest.raises(ValueError, match="fp16"):
        finetune_setup(shdr, precision="fp16", deterministic=True)
    K = shdr._ops
    x = torch.zeros((1, 4, 4, 16), device="cuda", dtype=torch.float16)
    with K.deterministic(True), pytest.raises(ValueError, match="fp16"):
        K.act_bwd_bias(x, None, K.ACT_NONE)


def test_switch_is_scoped_to_the_call(shdr):
    K = shdr._ops
    assert K.DETERMINISTIC is False
    step, _, ds, _ = per_net_run(shdr, "deq", True, iters=1)
    assert K.DETERMINISTIC is False
    with K.deterministic(True):
        assert K.DETERMINISTIC is True
        with K.deterministic(False):
            assert K.DETERMINISTIC is False
        step(ds, apply=False)
        assert K.DETERMINISTIC is True
        before = K.order_dependent_launches()                         # the ambient switch reaches a bare op
        K.bias_grad(torch.ones((4, 64, 64, 16), device="cuda"))
        assert K.order_dependent_launches() == before
    before = K.order_dependent_launches()
    K.bias_grad(torch.ones((4, 64, 64, 16), device="cuda"))
    assert K.order_dependent_launches() == before + 1
    assert K.DETERMINISTIC is False
