"""Every launch of tape-free inference against its float64 local reference (tests/inference_replay.py).

One recorded `torch.no_grad()` forward pass per test at the smallest shapes the nets accept and at one shape ragged against the kernels'
tiles.  Per pass: every launch within the project's op-level bar, fed the device's own operands; every derived operand (folded BatchNorm,
padded filters, the composed Hallucination tail and its projections) within its counted bar of the float64 formula from the variables;
every range a split-operand launch consumed bounds the tensor it was consumed for (kernel-written slots equal its maximum); the chain of
launches is closed; every C ABI call belongs to a recorded launch; the output still meets the whole-net bar.  Three planted errors show
that each check can fail, at exactly the places it should.
"""
import os

import numpy as np
import pytest
import torch

import inference_replay as IR
import test_gpu_fp16_inference as TF
import test_gpu_nets as TN
import test_gpu_tape_replay as TG
from conftest import GOLDEN, quantised_image, rel_err
from oracle import nets

pytestmark = pytest.mark.gpu

MODS = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
SEEDS = dict(deq=121, lin=122, hal=123, ref=124)
UNET_SHAPES = [(2, 32, 96), (1, 96, 160)]          # (1, 96, 160): u1's low-res input is 48 x 80 -- 8 row tiles of 6, 5 column tiles of 14 and one of 10
LIN_SHAPES = [(2, 64, 64), (1, 96, 128)]
CHAIN_SHAPES = [(2, 64, 96), (1, 96, 160)]
LAWS = ["dark", "bright_top"]

# C ABI entry points that may be called outside every recorded launch during a tape-free forward pass, each with its reason.
ALLOWED_OUTSIDE = {}

# K.RANGE_MISSES of one tape-free pass in the PLANNED configuration (fp32, default switches), input declared in [0, 1], as the parent commit
# shows them, by (x channels, x2 channels, filter shape).  A miss costs one pass over the tensor, so a new one fails the test.
U3_CONV1 = (128, None, (3, 3, 128, 64))      # u3.conv1 of the two U-Nets: the one-launch low-res form of the `up` block asks for a range ...
U2_CONV1 = (64, None, (3, 3, 64, 32))        # u2.conv1: ... and its producer (u4.conv2 / u3.conv2) runs a Winograd plan here, which writes none
HAL_D1_CONV1 = (4, None, (3, 3, 4, 64))      # hal.d1.conv1 in the chain: its input is vgg_preprocess(B_pred), and apply_rf hands no bound on
REF_CONV1 = (12, None, (7, 7, 12, 16))       # ref.conv1 in the chain: pack3([A, B, C]) has a bound only if all three sources have one
PLANNED_MISSES = {"deq": {U3_CONV1, U2_CONV1}, "ref": {U3_CONV1, U2_CONV1}, "lin": set(), "hal": set(), "chain": {U3_CONV1, U2_CONV1}}
# ... and with the split-operand plans forced (the benchmark's plans; every producer then writes its range): a net alone measures nothing,
# the chain measures the two inputs that arrive without a host bound.
SPLIT_FORCED_MISSES = {"deq": set(), "ref": set(), "lin": set(), "hal": set(), "chain": {HAL_D1_CONV1, REF_CONV1}}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def image(law, shape, seed):
    """the three input laws: quantised_image; the same times 2^-6 (every range far below 1); the same with its top third exactly 1.0 (the
    alpha mask is live over a region and B_pred reaches its clip)"""
    x = quantised_image(np.random.default_rng(seed), tuple(shape) + (3,))
    if law == "dark":
        x = x * 2.0 ** -6
    elif law == "bright_top":
        x[:, :shape[1] // 3] = 1.0
    return x


_MODELS = {}


def model_of(shdr, name, seed=None, fresh=False):
    """(model, oracle parameters); built once per (net, seed) -- the per-version caches on the model and its filters stay valid"""
    seed = SEEDS[name] if seed is None else seed
    if fresh or (name, seed) not in _MODELS:
        p = nets.init_params(getattr(nets, name + "_spec")(), seed)
        built = (getattr(shdr, MODS[name]).model().load_numpy(p), p)
        if fresh:
            return built
        _MODELS[(name, seed)] = built
    return _MODELS[(name, seed)]


@pytest.fixture(params=["exact_fp32", "fp16"])
def mode(request, monkeypatch, shdr):
    """the arms beside the `split_forced` fixture's two: K.EXACT_FP32 and precision="fp16"; -> the precision to run under"""
    if request.param == "exact_fp32":
        monkeypatch.setattr(shdr._ops, "EXACT_FP32", True)
    return "fp16" if request.param == "fp16" else "fp32"


def record_pass(shdr, fn, precision="fp32"):
    K = shdr._ops
    with torch.no_grad(), K.precision(precision), IR.record(K, audit=True) as rec:
        out = fn()
    rec.audit.finish()
    return rec, out


def miss_keys(counter):
    """(x shape, x2 shape or None, filter shape) of K.RANGE_MISSES -> (x channels, x2 channels or None, filter shape)"""
    return {(k[0][3], None if k[1] is None else k[1][3], tuple(k[2])) for k in counter}


def check_pass(shdr, rec, models, inputs, what):
    """the per-pass assertions of the module docstring but the whole-net bar; prints the figures DESIGN.md section 4.10 quotes"""
    rep = IR.replay(rec)
    entries, unresolved = IR.derived_report(rec, models)
    aud = rec.audit
    print("\n%s: %d launches (%d with nested ones), %d comparisons, %d derived operands, %d range consumptions, misses %s\n%s\nclosest to their bars:\n%s\n%s" % (
        what, len(rec.launches), len(list(rec.all())), len(rep.entries), len(entries), len(aud.items), dict(aud.misses()), rep.summary(),
        rep.closest(), aud.summary()))
    for l in rec.launches:
        if IR.is_fp16_tail(l):
            (e,) = [e for e in rep.entries if e.idx == l.idx]
            terms = IR.conv_terms({k: (IR.widen(v) if torch.is_tensor(v) else v) for k, v in l.a.items()})
            print("fp16 composed tail #%d: |err| %.3e = %.3e of the reference's maximum %.3e = %.3e of the largest sum of |terms| %.3e" % (
                l.idx, e.err, e.rel, e.ref_max, e.err / terms, terms))
            # beside the measured bar, the bound of the format: the operands are the fp16 values the tensors hold, the packed filter is
            # rounded to fp16 once (2^-11 per weight), accumulation and epilogue are fp32
            assert e.err <= 2.0 ** -11 * terms, (e.line(), terms)
    rep.assert_ok()
    assert not unresolved, ["%r.%s" % u for u in unresolved]
    assert all(e.ok for e in entries), "\n".join(e.line() for e in entries if not e.ok)
    aud.assert_sound()
    gaps = IR.open_inputs(rec, inputs)
    assert not gaps, ["%r.%s" % g for g in gaps]
    assert rec.abi_names() and set(rec.outside) <= set(ALLOWED_OUTSIDE), sorted(set(rec.outside) - set(ALLOWED_OUTSIDE))
    return rep, entries


def check_misses(rec, name, split_forced, mode="fp32"):
    if mode != "fp32":
        return
    got = miss_keys(rec.audit.misses())
    want = (SPLIT_FORCED_MISSES if split_forced else PLANNED_MISSES)[name]
    assert got <= want, "new range miss(es) in %s (x channels, x2 channels, filter shape): %s; all of this pass: %s" % (
        name, sorted(got - want, key=str), dict(rec.audit.misses()))


def net_case(shdr, name, x, precision="fp32", seed=None):
    """one recorded pass of one net on x (declared in [0, 1] as pipeline inputs are); -> (rec, output, model, parameters, device inputs).
    The Refinement-Net takes its three images packed as pipeline.Inference packs them: 12 fp32 channels, or 16 fp16 channels in native fp16"""
    K = shdr._ops
    m, p = model_of(shdr, name, seed)
    if name == "ref":
        xs = [K.set_bound(dev(x[..., 3 * i:3 * i + 3]), 1.0) for i in range(3)]
        rec, y = record_pass(shdr, lambda: m(K.pack3(xs, 16, K.HALF) if precision == "fp16" else K.pack3(xs, 12), training=False), precision)
        return rec, y, m, p, xs
    xd = K.set_bound(dev(x), 1.0)
    rec, y = record_pass(shdr, lambda: m(xd, training=False), precision)
    return rec, y, m, p, [xd]


def whole_net_bar(got, ref, precision):
    """the whole-net bars of tests/test_gpu_nets.py (fp32) and tests/test_gpu_fp16_inference.py (fp16), at a new shape"""
    err = rel_err(host(got), ref)
    print("whole net: %.3e of the reference's maximum" % err)
    assert err <= (TF.NET_TOL if precision == "fp16" else TN.TOL), err


def unet_input(name, law, shape, seed):
    if name != "ref":
        return image(law, shape, seed)
    return np.concatenate([image(law, shape, seed + i) for i in range(3)], axis=-1)                                     # [A, B, C]


def oracle_of(name, p, x, table=None):
    if name == "lin":
        return nets.lin_forward(p, x, table)
    return getattr(nets, name + "_forward")(p, x)


def run_net(shdr, name, law, shape, precision="fp32", split_forced=False, table=None, seed=5):
    x = unet_input(name, law, shape, seed)
    rec, y, m, p, xd = net_case(shdr, name, x, precision)
    exact = shdr._ops.EXACT_FP32
    check_pass(shdr, rec, {name: m}, xd, "%s %s %s %s%s" % (name, law, shape, "exact fp32" if exact else precision, " split-forced" if split_forced else ""))
    whole_net_bar(y, oracle_of(name, p, x, table), precision)
    check_misses(rec, name, split_forced, "exact" if exact else precision)
    return rec


# ---- the four nets: planned / split-forced, exact fp32 / fp16, the A/B switches, the input laws --------------------------------------------
@pytest.mark.parametrize("shape", UNET_SHAPES, ids=str)
@pytest.mark.parametrize("name", ["deq", "hal", "ref"])
def test_net_replay(shdr, split_forced, name, shape):
    rec = run_net(shdr, name, "quantised", shape, split_forced=split_forced)
    ops_seen = {l.op for l in rec.all()}
    if name == "hal":
        assert {"conv2d_maxpool2", "conv2d_up2", "vgg_preprocess", "fork"} <= ops_seen
        assert any(l.a["x2"] is not None and abs(l.a["x2_scale"] - 1.0 / 255) < 1e-9 for l in rec.of("conv2d"))          # the skip layers
        projected = [l for l in rec.launches if l.projected]
        print("projected launches:", projected)
        assert (len(projected) > 0) == bool(split_forced) and len(rec.of("affine_act")) == (1 if len(projected) == 2 else 0)   # d1.conv2 and u1
    else:
        assert {"conv2d_avgpool2", "conv2d_up2", "pack3"} <= ops_seen
        head = rec.of("conv2d")[-1]
        assert head.a["cout_valid"] == 3 and head.a["w"].shape[3] == 16 and head.a["residual"] is not None               # the fused heads


@pytest.mark.parametrize("shape", UNET_SHAPES, ids=str)
@pytest.mark.parametrize("name", ["deq", "hal", "ref"])
def test_net_replay_exact_fp32_and_fp16(shdr, mode, name, shape):
    rec = run_net(shdr, name, "quantised", shape, precision=mode)
    convs = [l for l in rec.launches if IR.OPS[l.op].conv]
    assert any(l.dtype == torch.float16 for l in convs) == (mode == "fp16") and all(l.prec == mode for l in rec.launches)
    if mode == "fp16":
        assert any(l.outs[0].dtype == torch.float32 and l.a["cout_valid"] == 3 for l in rec.of("conv2d"))                # the fp32 3-channel heads


@pytest.mark.parametrize("shape", UNET_SHAPES, ids=str)
@pytest.mark.parametrize("name,switch", [("deq", "SHDR_NO_UP2_NARROW"), ("hal", "SHDR_NO_UP2_FUSED")])
def test_net_replay_with_the_low_res_forms_switched_off(shdr, monkeypatch, split_forced, name, switch, shape):
    """the switches only move layers between kernels: the same bars"""
    monkeypatch.setenv(switch, "1")
    run_net(shdr, name, "quantised", shape, split_forced=split_forced)


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("name", ["deq", "hal", "ref"])
def test_net_replay_input_laws(shdr, split_forced, name, law):
    run_net(shdr, name, law, UNET_SHAPES[0], split_forced=split_forced)


@pytest.mark.parametrize("shape", LIN_SHAPES, ids=str)
def test_linearization_net_replay(shdr, emor_table, split_forced, shape):
    rec = run_net(shdr, "lin", "quantised", shape, split_forced=split_forced, table=emor_table)
    assert {"lin_frontend", "maxpool3s2", "global_avg_pool", "invcrf_decode", "increase", "fork"} <= {l.op for l in rec.launches}
    joins = [l for l in rec.of("conv2d") if l.a["residual"] is not None]
    assert len(joins) == 5 and all(l.a["scale"] is not None and l.a["act2"] == 1 for l in joins)                         # the fused residual joins
    stem = rec.of("conv2d")[0]
    assert stem.a["x"].shape[3] == 96 and stem.a["stride"] == 2 and stem.a["cout_valid"] == 64


@pytest.mark.parametrize("shape", LIN_SHAPES, ids=str)
def test_linearization_net_replay_exact_fp32(shdr, emor_table, monkeypatch, shape):
    monkeypatch.setattr(shdr._ops, "EXACT_FP32", True)
    run_net(shdr, "lin", "quantised", shape, table=emor_table)


@pytest.mark.parametrize("law", LAWS)
def test_linearization_net_replay_input_laws(shdr, emor_table, split_forced, law):
    run_net(shdr, "lin", law, LIN_SHAPES[0], split_forced=split_forced, table=emor_table)


# ---- the full chain ----------------------------------------------------------------------------------------------------------------------
def chain_case(shdr, table, law, shape, precision, what, golden_seeds):
    K = shdr._ops
    seeds = SEEDS
    if golden_seeds:
        g = np.load(os.path.join(GOLDEN, "inference_64.npz"))
        seeds = {k: int(g["seed_" + k]) for k in MODS}
    built = {k: model_of(shdr, k, seeds[k]) for k in MODS}
    ms = {k: v[0] for k, v in built.items()}
    x = image(law, shape, 6)
    xd = K.set_bound(dev(x), 1.0)
    run = shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision=precision)
    with IR.record(K, audit=True) as rec:
        out = run(xd, return_intermediates=True)
    rec.audit.finish()
    check_pass(shdr, rec, ms, [xd], "chain %s %s %s" % (law, shape, what))
    ref = nets.inference({k: v[1] for k, v in built.items()}, x, table)
    errs = {key: rel_err(host(out[key]), ref[key]) for key in ("C_pred", "invcrf", "B_pred", "hal", "A_pred", "hdr")}
    print("whole chain:", {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) <= (TF.NET_TOL if precision == "fp16" else TN.TOL), errs
    return rec, out


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=str)
def test_inference_chain_replay(shdr, emor_table, split_forced, shape):
    rec, _ = chain_case(shdr, emor_table, "quantised", shape, "fp32", "split-forced" if split_forced else "planned", shape == CHAIN_SHAPES[0])
    check_misses(rec, "chain", split_forced)
    assert {"clip", "apply_rf", "alpha_blend", "pack3", "lin_frontend"} <= {l.op for l in rec.launches}


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=str)
def test_inference_chain_replay_exact_fp32_and_fp16(shdr, emor_table, mode, shape):
    rec, _ = chain_case(shdr, emor_table, "quantised", shape, mode, "exact fp32" if shdr._ops.EXACT_FP32 else mode, shape == CHAIN_SHAPES[0])
    if mode == "fp16":
        (front,) = rec.of("lin_frontend")
        assert front.prec == "fp32" and front.outs[0].dtype == torch.float32                                             # the Linearization-Net stays fp32


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_inference_chain_replay_input_laws(shdr, emor_table, monkeypatch, law, precision):
    """the dark and the bright-top image through the whole chain, on the benchmark's plans (fp32: the split-operand kernels forced) and in
    native fp16"""
    if precision == "fp32":
        monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    _, out = chain_case(shdr, emor_table, law, CHAIN_SHAPES[0], precision, "fp16" if precision == "fp16" else "split-forced", True)
    if law == "bright_top":
        assert float(out["C_pred"].max()) == 1.0 and float(out["B_pred"].max()) > 1.0 - 1e-5                             # both reach the top of their range
        assert bool((out["A_pred"] != out["B_pred"]).any())                                                              # the alpha mask is live


# ---- the range audit on the training steps -------------------------------------------------------------------------------------------------
def audited_step(shdr, step_fn, what):
    K = shdr._ops
    with IR.audit_ranges(K) as aud:
        step_fn()
    aud.finish()
    print("\n%s: %d range consumptions, misses %s\n%s" % (what, len(aud.items), dict(aud.misses()), aud.summary()))
    assert len(aud.items) > 0
    aud.assert_sound()
    return aud


def test_joint_step_range_audit(shdr, split_forced):
    """forward and backward of one JointTrainStep at the shapes and seeds of tests/test_gpu_joint.py: the backward rules (|act'| <= 1, pool
    and resize gradients, dz handed to dgrad and wgrad) carry the most hand-written bounds"""
    rng = np.random.default_rng(11)
    ms, vgg = TG.three_nets(shdr, 70)
    batch, inv = TG.make_batch(rng, 3, 64)
    step = shdr.pipeline.JointTrainStep(ms["deq"], ms["lin"], ms["hal"], vgg, lr=1e-3)
    batch, inv = tuple(dev(t) for t in batch), dev(inv)
    aud = audited_step(shdr, lambda: step(batch, inv, apply=False), "joint step%s" % (" split-forced" if split_forced else ""))
    assert {"conv2d_wgrad"} <= {c.who for c in aud.items}
    if split_forced:
        assert {"_conv2d_raw", "conv2d_dgrad"} <= {c.who for c in aud.items}


def test_finetune_step_range_audit(shdr, split_forced):
    """tests/test_gpu_finetune.py::ft, fp32"""
    rng = np.random.default_rng(12)
    P = {k: nets.init_params(getattr(nets, k + "_spec")(), 95 + i) for i, k in enumerate(MODS)}
    ldr = quantised_image(rng, (2, 64, 64, 3))
    ldr[0, :12, :12] = 1.0
    hdr = rng.random((2, 64, 64, 3)) * 1.5
    hdr = hdr / (1e-6 + hdr.mean(axis=(1, 2, 3), keepdims=True)) * 0.5
    ms = {k: getattr(shdr, MODS[k]).model().load_numpy(P[k]) for k in MODS}
    step = shdr.pipeline.FinetuneStep(ms["deq"], ms["lin"], ms["hal"], ms["ref"], lr=1e-4)
    audited_step(shdr, lambda: step(dev(ldr), dev(hdr), apply=False), "fine-tune step%s" % (" split-forced" if split_forced else ""))


# ---- the replay must be able to fail -----------------------------------------------------------------------------------------------------
def test_control_folded_shift_with_the_wrong_sign(shdr, emor_table, monkeypatch):
    """BatchNormalization.folded returns shift = beta + mean scale: every folded shift the pass consumed is reported by the derived-operand
    check and nothing else is; no launch fails, because each launch is fed its own operands"""
    L = shdr._layers

    def wrong(self):
        with torch.no_grad():
            scale = self.gamma.detach() * torch.rsqrt(self.moving_variance + L.BN_EPS)
            self._folded = (None, scale.contiguous(), (self.beta.detach() + self.moving_mean * scale).contiguous())
        return self._folded[1], self._folded[2]
    monkeypatch.setattr(L.BatchNormalization, "folded", wrong)
    m, p = model_of(shdr, "lin", fresh=True)
    xd = shdr._ops.set_bound(dev(image("quantised", LIN_SHAPES[0], 7)), 1.0)
    rec, _ = record_pass(shdr, lambda: m(xd, training=False))
    IR.replay(rec).assert_ok()
    entries, unresolved = IR.derived_report(rec, {"lin": m})
    bad = {e.name for e in entries if not e.ok}
    want = {e.name for e in entries if e.name.endswith(".folded.shift")}
    assert not unresolved and len(want) == 18 and bad == want, sorted(bad ^ want)


def test_control_tail_join_drops_its_residual(shdr, monkeypatch):
    """K.affine_act without its residual: exactly the launch where the Hallucination tail's two projections meet fails"""
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")          # the split-operand plans: the tail's 64 -> 3 maps come out of the producers' epilogues
    orig = K.affine_act
    monkeypatch.setattr(K, "affine_act", lambda x, scale=None, shift=None, residual=None, act=0: orig(x, scale, shift, None, act))
    m, _ = model_of(shdr, "hal")
    xd = K.set_bound(dev(image("quantised", UNET_SHAPES[1], 8)), 1.0)
    rec, _ = record_pass(shdr, lambda: m(xd, training=False))
    (join,) = rec.of("affine_act")
    assert join.a["residual"] is not None
    rep = IR.replay(rec)
    assert rep.failed() == {(join.idx, "out[0]")}, "\n".join(e.line() for e in rep.failures())


def test_control_host_bounds_recorded_at_half(shdr, monkeypatch):
    """K.set_bound records half of every bound: the audit reports exactly the consumers of host bounds; the fp16 headroom of the
    split-operand kernels keeps every launch inside its bar"""
    K = shdr._ops
    monkeypatch.setenv("SHDR_X3_MIN_BLOCKS", "1")
    orig = K.set_bound
    monkeypatch.setattr(K, "set_bound", lambda t, bound: orig(t, 0.5 * bound))
    ms = {k: model_of(shdr, k)[0] for k in MODS}
    xd = K.set_bound(dev(image("bright_top", CHAIN_SHAPES[0], 9)), 1.0)
    run = shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"])
    with IR.record(K, audit=True) as rec:
        out = run(xd)
    aud = rec.audit.finish()
    print("\n".join(c.line() for c in aud.items if c.kind == "host"))
    hosts = [c for c in aud.items if c.kind == "host"]
    assert len(hosts) >= 1 and aud.failures() == hosts
    IR.replay(rec).assert_ok()
    assert bool(torch.isfinite(out).all())


# ---- graph replay under changing input laws ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_graphed_inference_replays_other_input_laws(shdr, precision):
    """captured on the bright-top image, replayed on the dark one, on quantised_image and on the bright one again: a constant or a range
    frozen into the graph at capture would show against eager inference on the same input"""
    ms = {k: model_of(shdr, k)[0] for k in MODS}
    eager = shdr.pipeline.Inference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision=precision)
    graphed = shdr.pipeline.GraphedInference(ms["deq"], ms["lin"], ms["hal"], ms["ref"], precision=precision)
    shape = (128, 96)
    for law in ("bright_top", "dark", "quantised", "bright_top"):
        x = dev(image(law, (1,) + shape, 10))
        np.testing.assert_array_equal(host(graphed(x)), host(eager(x)), err_msg=law)
