"""Every tape node of the training nets against its float64 local gradient (tests/tape_replay.py).

One recorded forward and backward pass per test at the smallest shapes the nets accept, with the seeds and inputs of the existing
whole-net tests (test_gpu_grad.py, test_gpu_finetune.py, test_gpu_joint.py, test_gpu_fp16_oracle.py).  Each node is fed the device's
own inputs and upstream gradient, so a relu / max-pool / `_increase` mask that flips against a float64 forward is no excuse here: the
op-level bars (1e-5 forward, 1e-4 gradients, 2e-4 CRF head; fp16: 2e-3 / 3e-3 conv, one fp16 ulp elementwise) hold for EVERY node, no
element is excluded, and every variable's gradient buffer must equal the sum of the float64 local gradients of the nodes that consume
it (the `_acc` fast path adds into the flat buffer and returns None).  Three planted errors show that the replay can fail, each
reported at exactly its nodes or variables.
"""
import numpy as np
import pytest
import torch

import fp16_ref as H
import tape_ref as TR
import tape_replay as TP
import torch_ref as R
from conftest import quantised_image
from oracle import nets

pytestmark = pytest.mark.gpu

# Backward nodes that are not a recorded Function and may sit between the loss and the leaves: plumbing on parameter-sized or [b]-sized
# tensors, never a feature map.
ALLOWED_FOREIGN = {
    "AccumulateGrad": "the leaves",
    "SumBackward0": "the sum that closes the loss (over the [b] / [b,1,b,1] loss tensor)",
    "MulBackward0": "per-sample loss [b] times loss_mask / a scalar weight (pipeline.py: `* mask`, `10.0 * l2_lin`, `b_glob * ...`)",
    "AddBackward0": "sum of per-sample loss terms [b] (perceptual + l1 + tv; deq + lin + hal)",
    "ConstantPadNdBackward0": "Conv2D.call_padded: F.pad of a narrow FILTER to the MFMA tile (parameter-sized)",
}
# Edges where a recorded output that required grad arrives at a recorded consumer as a constant.  The reference's own stop-gradients
# are all taken on DATA, in front of the tape (the alpha mask of joint_training.py:141-145 / train.py:209-213 is computed from
# clipped_hdr_t, the perceptual target features of joint_training.py:168-170 from hdr_t under no tape), so no recorded edge is cut.
EXPECTED_CUTS = []
# Recorded outputs handed as ONE object to several recorded consumers (autograd's own add then sums their gradients instead of ForkFn's
# kernel): the Refinement-Net reads its packed input twice -- the first 7x7 layer and the residual slice (refinement_net.py:26-28).
REF_INPUT_FANOUT = ("Pack3Fn", ("Conv2dFn", "Unpack3Fn"))
REF_INPUT_FANOUT_H = ("Pack3Fn", ("Conv2dHFn", "Unpack3Fn"))
# ... the predicted inverse CRF feeds apply_rf and the crf loss (pipeline.py: JointTrainStep.losses, TrainStep.forward "lin") ...
INVCRF_FANOUT = ("IncreaseFn", ("ApplyRfFn", "DiffLossFn"))
# ... and the per-network Hallucination step hands log(A) to the perceptual, L1 and TV terms without the fork the joint step has
HAL_LOSS_FANOUT = ("LogcFn", ("DiffLossFn", "TvLossFn", "VggPreFn"))


def dev(x, grad=False):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


def named(prefix, model):
    return [(prefix + n, t) for n, t, tr in model.named_weights() if tr]


def plan_of(K):
    def plan(node):
        if node.name == "Conv2dHFn":
            return "fp16"
        if node.name != "Conv2dFn":
            return None
        x, x2, w, _, stride, x2_scale, _, cout_valid = node.args[:8]
        try:
            p = K.conv2d_plan(tuple(x.shape), tuple(w.shape), 0 if x2 is None else x2.shape[3], stride, x2_scale, False, cout_valid)
        except Exception:       # the plan is for the report only
            p = "?"
        return "%s/%s" % (p, node.prec)
    return plan


def recorded(shdr, fn, variables, grad_scale=1.0, fanouts=()):
    """run fn under the recorder, replay, print the per-class figures, check the structure; returns (rec, rep, fn's result)"""
    A, K = shdr._autograd, shdr._ops
    for _, t in variables:
        if not getattr(t, "_shdr_accum", False):
            t.grad = None
    with TP.record(A) as rec:
        out = fn()
    torch.cuda.synchronize()
    rep = TP.replay(rec, variables, grad_scale, plan_of(K))
    found, cuts, fans = TP.foreign_nodes(rec), TP.cut_edges(rec), TP.unforked_fanouts(rec)
    print("\n%d nodes, %d comparisons; foreign %s; cuts %s; unforked fan-outs %s\n%s\nclosest to their bars:\n%s" % (
        len(rec.nodes), len(rep.entries) + len(rep.var_entries), found, cuts, fans, rep.summary(), rep.closest()))
    assert set(found) <= set(ALLOWED_FOREIGN), sorted(set(found) - set(ALLOWED_FOREIGN))
    assert cuts == EXPECTED_CUTS, cuts
    assert fans == sorted(fanouts), fans
    reached = {t.data_ptr() for t in TP.reached_variables(rec)}
    assert all(t.data_ptr() in reached for _, t in variables), [n for n, t in variables if t.data_ptr() not in reached]
    assert all(n.hook_calls <= 1 for n in rec.nodes)
    return rec, rep, out


def classes(rec):
    return {n.name for n in rec.nodes}


# ---- 1. the four nets with training=True --------------------------------------------------------------------------------------------
def deq_case(shdr):
    """test_gpu_grad.py::test_dequantization_net_gradients"""
    K = shdr._ops
    p = nets.init_params(nets.deq_spec(), 61)
    m = shdr.dequantization_net.model().load_numpy(p)
    rng = np.random.default_rng(1)
    x, tgt = quantised_image(rng, (2, 32, 32, 3)), quantised_image(rng, (2, 32, 32, 3))
    return p, m, x, tgt, lambda: K.diff_loss(K.clip(m(dev(x), training=True), 0.0, 1.0), dev(tgt), 0).sum().backward()


def test_dequantization_net_tape(shdr):
    _, m, _, _, run = deq_case(shdr)
    rec, rep, _ = recorded(shdr, run, named("", m))
    rep.assert_ok()
    assert {"Conv2dFn", "AvgPool2Fn", "Resize2xFn", "AddFn", "ForkFn", "ClipFn", "DiffLossFn"} <= classes(rec)
    assert any(n.args[1] is not None for n in rec.of("Conv2dFn"))                  # the two-source layers of the up blocks


STEM_BIAS = "crf_feature_net.conv1.bias"


def is_stem_bias(e):
    """the gradient of the Linearization-Net's stem bias: the variable's comparison and, where the node returns it, the node's"""
    return e.item == STEM_BIAS or (e.name == "Conv2dFn" and e.idx == 0 and e.item == "grad[3]")


def stem_bias_figures(rec, rep):
    """prints the error of the stem bias gradient's worst channel in units of u sum|dz| (u = 2^-24) beside the figure the bar sees, and
    holds it to the fp32 summation bound of tape_ref.sum_bar"""
    stem = rec.of("Conv2dFn")[0]
    dz = H.act_grad(TP.widen(stem.grad_outputs[0]), TP.widen(stem.outs[0]), stem.args[6])
    (e,) = [e for e in rep.var_entries if e.item == STEM_BIAS]
    mags = np.abs(dz).reshape(-1, dz.shape[-1]).sum(axis=0)
    gmax, ch = e.floor / TP.MODEL_SCALE, e.where[0]
    print("%s: |err| %.3e = %.2f u sum|dz| in channel %d (sum|dz| = %.3e = %.1f x the model-wide maximum gradient %.3e); the bar's "
          "figure: %.3e of 1e-4, i.e. the bar allows %.2f u sum|dz|" % (STEM_BIAS, e.err, e.err / (TR.U32 * mags[ch]), ch, mags[ch],
                                                                      mags[ch] / gmax, gmax, e.rel, e.bar * e.floor / (TR.U32 * mags[ch])))
    assert e.err <= float(TR.sum_bar(dz.reshape(-1, dz.shape[-1]), axis=0)[ch])


@pytest.fixture(scope="module")
def lin_alone(shdr, emor_table):
    """test_gpu_grad.py::test_linearization_net_gradients_training_bn, recorded and replayed once"""
    K = shdr._ops
    m = shdr.linearization_net.model().load_numpy(nets.init_params(nets.lin_spec(), 62))
    rng = np.random.default_rng(2)
    x = quantised_image(rng, (2, 64, 64, 3))
    inv = np.cumsum(rng.random((2, 1024)), axis=1)
    inv /= inv[:, -1:]
    rec, rep, _ = recorded(shdr, lambda: K.diff_loss(m(dev(x), training=True), dev(inv), 0).sum().backward(), named("", m))
    return rec, rep


def test_linearization_net_tape_training_bn(lin_alone):
    """every comparison but the stem bias gradient, which test_linearization_stem_bias_gradient_on_the_model_wide_scale asserts"""
    rec, rep = lin_alone
    rep.assert_ok(leave=is_stem_bias)
    assert {"Conv2dFn", "BatchNormTrainFn", "MaxPool3s2Fn", "AddReluFn", "GapFn", "InvcrfDecodeFn", "IncreaseFn"} <= classes(rec)
    stem = rec.of("Conv2dFn")[0]
    assert stem.args[0].shape[3] == 96 and stem.args[2].shape[2] == 96 and stem.args[4] == 2          # the 93 -> 96 stem, 7x7 / 2
    assert TP.variable_of(stem.args[2]).shape[2] == 93


@pytest.mark.parametrize("where", ["net", "train_step"])
def test_linearization_stem_bias_gradient_on_the_model_wide_scale(request, where):
    """`crf_feature_net.conv1.bias` sits in front of a training-mode BatchNorm: its true gradient is zero, the device's is the sum of
    2048 cancelling terms per channel, and it is measured against 1e-3 of the model-wide maximum gradient (as _grad_check does), bar
    1e-4 -- which allows 0.36 .. 0.57 u sum|dz| of the worst channel (u = 2^-24), less than one fp32 rounding of the sum of magnitudes.
    With fp32 sums and fp32 atomics over the blocks (the parent's act_bwd_bias_kernel) the error was 0.25 .. 0.85 u sum|dz|: 5.4e-5 ..
    1.484e-4 against the bar, over it in 5 of 12 runs.  The kernel now sums in double and folds the blocks' rows in double
    (csrc/bwd.hip, shdr_internal.h: col_fold_kernel); measured since: 1.2e-5 in both tapes, 0.05 .. 0.06 u sum|dz|.  Asserted here, apart from the other comparisons
    of the two Linearization-Net tapes, so that a miss names it."""
    rec, rep = request.getfixturevalue({"net": "lin_alone", "train_step": "lin_step"}[where])
    stem_bias_figures(rec, rep)
    bad = [e for e in rep.entries + rep.var_entries if is_stem_bias(e) and not e.ok]
    assert not bad, "\n".join(e.line() for e in bad)


def test_hallucination_net_tape_training_bn(shdr):
    """test_gpu_grad.py::test_hallucination_net_gradients_training_bn"""
    K = shdr._ops
    m = shdr.hallucination_net.model().load_numpy(nets.init_params(nets.hal_spec(), 63))
    rng = np.random.default_rng(3)
    x, tgt = quantised_image(rng, (2, 64, 64, 3)), rng.random((2, 64, 64, 3))
    rec, rep, _ = recorded(shdr, lambda: K.diff_loss(m(dev(x), training=True), dev(tgt), 1).sum().backward(), named("", m))
    rep.assert_ok()
    assert {"Conv2dFn", "BatchNormTrainFn", "MaxPool2Fn", "Resize2xFn"} <= classes(rec)
    assert any(abs(n.args[5] - 1.0 / 255) < 1e-9 and n.args[1] is not None for n in rec.of("Conv2dFn"))    # the skips, x2_scale 1 / 255


def test_refinement_net_tape(shdr):
    """test_gpu_finetune.py::test_refinement_net_gradients"""
    K = shdr._ops
    m = shdr.refinement_net.model().load_numpy(nets.init_params(nets.ref_spec(), 91))
    rng = np.random.default_rng(4)
    x = rng.random((2, 32, 32, 9))
    tgt = rng.random((2, 32, 32, 3))
    x12 = dev(np.concatenate([x, np.zeros((2, 32, 32, 3))], -1), True)
    rec, rep, _ = recorded(shdr, lambda: K.diff_loss(m(x12, training=True), dev(tgt), 1).sum().backward(), named("", m))
    rep.assert_ok()
    assert {"Conv2dFn", "Unpack3Fn", "AddReluFn"} <= classes(rec) and rep.other_leaves == 1        # the input: a leaf, no variable
    head = rec.of("Conv2dFn")[-1]
    assert head.args[7] == 3 and head.args[2].shape[3] == 16                                       # cout_valid 3 of 16


# ---- 2. training=False under a tape ------------------------------------------------------------------------------------------------------
def test_frozen_batchnorm_tapes(shdr, emor_table):
    """test_gpu_grad.py::test_inference_mode_networks_under_a_tape: the moving statistics are constants, gamma / beta and the filters train"""
    K = shdr._ops
    rng = np.random.default_rng(5)
    m = shdr.linearization_net.model().load_numpy(nets.init_params(nets.lin_spec(), 64))
    x = quantised_image(rng, (2, 64, 64, 3))
    inv = np.cumsum(rng.random((2, 1024)), axis=1)
    inv /= inv[:, -1:]
    rec, rep, _ = recorded(shdr, lambda: K.diff_loss(m(dev(x), training=False), dev(inv), 0).sum().backward(), named("", m))
    rep.assert_ok()
    assert classes(rec) & {"BatchNormFrozenFn", "AffineActFn"} and "BatchNormTrainFn" not in classes(rec)
    m = shdr.hallucination_net.model().load_numpy(nets.init_params(nets.hal_spec(), 65))
    x, tgt = quantised_image(rng, (1, 64, 64, 3)), rng.random((1, 64, 64, 3))
    rec, rep, _ = recorded(shdr, lambda: K.diff_loss(m(dev(x), training=False), dev(tgt), 1).sum().backward(), named("", m))
    rep.assert_ok()
    assert classes(rec) & {"BatchNormFrozenFn", "AffineActFn"} and "BatchNormTrainFn" not in classes(rec)


def test_affine_epilogue_and_mark_tapes(shdr):
    """the two Function classes no training step records on one GPU: AffineActFn (a fused inference epilogue -- folded BatchNorm, residual,
    second activation -- asked for under a tape: conv + affine entries) and MarkFn (the data-parallel steps' bucket mark)"""
    K = shdr._ops
    rng = np.random.default_rng(6)
    x, res = dev(rng.normal(size=(2, 9, 7, 16)), True), dev(rng.normal(size=(2, 9, 7, 32)), True)
    w, b = dev(rng.normal(size=(3, 3, 16, 32)) / 12.0, True), dev(rng.normal(size=32) * 0.1, True)
    scale, shift = dev(rng.uniform(0.5, 1.5, 32)), dev(rng.normal(size=32))
    tgt = dev(rng.normal(size=(2, 9, 7, 32)))
    calls = []

    def run():
        y = K.conv2d(x, w, b, act1=K.ACT_LRELU, scale=scale, shift=shift, residual=res, act2=K.ACT_RELU)
        z = K.affine_act(K.mark(y, lambda: calls.append(1)), None, None, res, K.ACT_TANH)
        K.diff_loss(z, tgt, 0).sum().backward()
    rec, rep, _ = recorded(shdr, run, [("w", w), ("b", b)])
    rep.assert_ok()
    assert [n.name for n in rec.nodes] == ["Conv2dFn", "AffineActFn", "MarkFn", "AffineActFn", "DiffLossFn"] and calls == [1]
    assert rep.other_leaves == 2 and x.grad is not None and res.grad is not None


# ---- 3. the joint step: flat parameters, the `_acc` path ---------------------------------------------------------------------------------
def make_batch(rng, b, s):
    """tests/test_gpu_joint.py::make_batch"""
    clipped = quantised_image(rng, (b, s, s, 3))
    clipped[0, :10, :10] = 1.0
    hdr_t = clipped * np.where(clipped >= 1.0, 1 + 3 * rng.random((b, s, s, 3)), 1.0)
    inv = np.cumsum(rng.random((b, 1024)), axis=1)
    inv = (inv - inv[:, :1]) / (inv[:, -1:] - inv[:, :1])
    mask = np.ones((b, 1, 1, 1))
    mask[-1] = 0.0
    return (quantised_image(rng, (b, s, s, 3)), quantised_image(rng, (b, s, s, 3)), clipped, hdr_t, mask), inv


def three_nets(shdr, seed):
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net")
    P = {k: nets.init_params(getattr(nets, k + "_spec")(), seed + i) for i, k in enumerate(mods)}
    V = nets.init_params(nets.vgg_spec(), seed + 3)
    ms = {k: getattr(shdr, mods[k]).model().load_numpy(P[k]) for k in mods}
    dd = {n: [V[n + ".kernel"], V[n + ".bias"]] for n in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3")}
    return ms, shdr.vgg16.Vgg16(data_dict=dd)


@pytest.fixture(scope="module")
def joint(shdr):
    """tests/test_gpu_joint.py::setup"""
    rng = np.random.default_rng(11)
    ms, vgg = three_nets(shdr, 70)
    batch, inv = make_batch(rng, 3, 64)
    step = shdr.pipeline.JointTrainStep(ms["deq"], ms["lin"], ms["hal"], vgg, lr=1e-3)
    return dict(step=step, ms=ms, batch=tuple(dev(t) for t in batch), inv=dev(inv))


def test_joint_step_tape(shdr, joint, split_forced):
    step = joint["step"]
    variables = [v for k in ("deq", "lin", "hal") for v in named(k + ".", joint["ms"][k])]
    assert [t.data_ptr() for _, t in variables] == [t.data_ptr() for t in step.params.variables]
    rec, rep, _ = recorded(shdr, lambda: step(joint["batch"], joint["inv"], apply=False), variables, fanouts=[INVCRF_FANOUT])
    rep.assert_ok()
    assert {"BlendConstFn", "LogcFn", "TvLossFn", "ApplyRfFn", "ForkFn", "DiffLossFn"} <= classes(rec)
    # every filter and BatchNorm vector went through the `_acc` path: the nodes returned no gradient for them
    acc = [n for n in rec.of("Conv2dFn") if getattr(n.args[2], "_shdr_accum", False) and n.grad_outputs is not None]
    assert len(acc) > 50 and all(n.aligned_grad_inputs()[2] is None for n in acc)
    if split_forced:
        assert any("x3" in e.plan for e in rep.entries if e.name == "Conv2dFn")


# ---- 4. the per-network steps ------------------------------------------------------------------------------------------------------------
def train_step_tape(shdr, which):
    """tests/test_gpu_joint.py::test_per_network_train_steps_match_the_joint_pieces"""
    rng = np.random.default_rng(21)
    ms, vgg = three_nets(shdr, 80)
    batch, inv = make_batch(rng, 2, 64)
    ldr, jpeg, clipped, hdr_t, mask = (dev(t) for t in batch)
    step = shdr.pipeline.TrainStep(which, ms[which], vgg if which == "hal" else None)
    ds = {"deq": (ldr, jpeg, mask), "lin": (ldr, clipped, mask, dev(inv)), "hal": (hdr_t, clipped, mask)}[which]
    fan = {"deq": [], "lin": [INVCRF_FANOUT], "hal": [HAL_LOSS_FANOUT]}[which]
    rec, rep, _ = recorded(shdr, lambda: step(ds, apply=False), named("", ms[which]), fanouts=fan)
    return rec, rep


@pytest.fixture(scope="module")
def lin_step(shdr):
    return train_step_tape(shdr, "lin")


@pytest.mark.parametrize("which", ["deq", "lin", "hal"])
def test_per_network_train_step_tapes(shdr, request, which):
    """lin: every comparison but the stem bias gradient (test_linearization_stem_bias_gradient_on_the_model_wide_scale)"""
    rec, rep = request.getfixturevalue("lin_step") if which == "lin" else train_step_tape(shdr, which)
    rep.assert_ok(leave=is_stem_bias if which == "lin" else None)
    assert all(getattr(n.args[2], "_shdr_accum", False) or TP.variable_of(n.args[2]) is not n.args[2] for n in rec.of("Conv2dFn")
               if n.arg_requires_grad[2])                   # every trainable filter sits in the flat buffer or is the padded view of one


# ---- 5. the chained fine-tuning step, fp32 and native fp16 -------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_finetune_step_tape(shdr, precision):
    """tests/test_gpu_finetune.py::ft, tests/test_gpu_fp16_oracle.py::ft16.  fp16: the loss scale 0.25 is part of the recorded upstream
    gradients; the step divides it out of the flat buffer, so the buffer is 1 / 0.25 times the sum of the local gradients"""
    rng = np.random.default_rng(12)
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    P = {k: nets.init_params(getattr(nets, k + "_spec")(), 95 + i) for i, k in enumerate(mods)}
    ldr = quantised_image(rng, (2, 64, 64, 3))
    ldr[0, :12, :12] = 1.0
    hdr = rng.random((2, 64, 64, 3)) * 1.5
    hdr = hdr / (1e-6 + hdr.mean(axis=(1, 2, 3), keepdims=True)) * 0.5
    ms = {k: getattr(shdr, mods[k]).model().load_numpy(P[k]) for k in mods}
    kw = dict(precision="fp16", loss_scale=0.25) if precision == "fp16" else {}
    step = shdr.pipeline.FinetuneStep(ms["deq"], ms["lin"], ms["hal"], ms["ref"], lr=1e-4, **kw)
    variables = [v for k in mods for v in named(k + ".", ms[k])]
    half = precision == "fp16"
    rec, rep, _ = recorded(shdr, lambda: step(dev(ldr), dev(hdr), apply=False), variables, grad_scale=1.0 / step.loss_scale,
                           fanouts=[REF_INPUT_FANOUT_H if half else REF_INPUT_FANOUT])
    assert step.skipped_steps == 0
    rep.assert_ok()
    assert {"LinFrontendFn", "AlphaBlendFn", "Pack3Fn", "Unpack3Fn", "MeanNormFn", "ApplyRfFn", "ForkFn"} <= classes(rec)
    assert ("Conv2dHFn" in classes(rec)) == half and all(n.prec == precision for n in rec.nodes)
    if half:
        assert any(n.outs[0].dtype == torch.float32 and n.args[7] == 3 for n in rec.of("Conv2dHFn"))     # the fp32 3-channel heads
        assert any(n.outs[0].dtype == torch.float16 for n in rec.of("BatchNormTrainFn"))                 # the fp16 elementwise twins


# ---- the replay must be able to fail ---------------------------------------------------------------------------------------------------
def test_control_second_source_input_gradient_off_by_a_thousandth(shdr, monkeypatch):
    """dx2 of every two-source layer times 1 + 1e-3: the replay names exactly those nodes' grad[1]; the whole-net gradient stays far
    inside the 2e-2 whole-net bar (test_gpu_grad.NET_L2_TOL) -- the gap the replay closes"""
    A = shdr._autograd
    p, m, x, tgt, run = deq_case(shdr)
    orig = A._dgrad
    monkeypatch.setattr(A, "_dgrad", lambda dz, w, which, *a: orig(dz, w, which, *a) * (1.0 + 1e-3) if which == 1 else orig(dz, w, which, *a))
    rec, rep, _ = recorded(shdr, run, named("", m))
    want = {(n.idx, "grad[1]") for n in rec.of("Conv2dFn") if n.args[1] is not None and n.aligned_grad_inputs()[1] is not None}
    assert len(want) >= 4 and rep.failed_items() == (want, set()), rep.text(True)
    tp = R.params_to_torch(p)
    (((torch.clamp(R.deq_forward(tp, R.T(x)), 0, 1) - R.T(tgt)) ** 2).mean(dim=(1, 2, 3))).sum().backward()
    ref = {n: tp[n].grad.numpy() for n, _ in named("", m)}
    gmax = max(float(np.abs(r).max()) for r in ref.values())
    worst = max(float(np.linalg.norm(host(t.grad) - ref[n]) / max(np.linalg.norm(ref[n]), 1e-3 * gmax * np.sqrt(ref[n].size))) for n, t in named("", m))
    print("whole-net gradient with the planted error: worst per-variable relative L2 = %.2e" % worst)
    assert 1e-5 < worst <= 2e-2, worst


def test_control_fork_drops_its_last_gradient(shdr, monkeypatch):
    A = shdr._autograd
    _, m, _, _, run = deq_case(shdr)
    orig = A.ForkFn.backward
    monkeypatch.setattr(A.ForkFn, "backward", staticmethod(lambda ctx, *gs: orig(ctx, *(gs[:-1] + (None,)))))
    rec, rep, _ = recorded(shdr, run, named("", m))
    want = {(n.idx, "grad[0]") for n in rec.of("ForkFn") if n.grad_outputs is not None and n.grad_outputs[-1] is not None}
    assert len(want) >= 4 and rep.failed_items() == (want, set()), rep.text(True)


def test_control_one_flat_buffer_slice_receives_its_weight_gradient_twice(shdr, monkeypatch):
    K = shdr._ops
    rng = np.random.default_rng(21)
    ms, _ = three_nets(shdr, 80)
    batch, _ = make_batch(rng, 2, 64)
    ldr, jpeg, _, _, mask = (dev(t) for t in batch)
    step = shdr.pipeline.TrainStep("deq", ms["deq"])
    variables = named("", ms["deq"])
    name, target = [(n, t) for n, t in variables if t.dim() == 4][5]
    orig = K.conv2d_wgrad

    def twice(x, x2, dz, w_shape, stride=1, x2_scale=1.0, out=None):
        if out is not None and out.data_ptr() == target.grad.data_ptr():
            orig(x, x2, dz, w_shape, stride, x2_scale, out=out)
        return orig(x, x2, dz, w_shape, stride, x2_scale, out=out)
    monkeypatch.setattr(K, "conv2d_wgrad", twice)
    rec, rep, _ = recorded(shdr, lambda: step((ldr, jpeg, mask), apply=False), variables)
    assert rep.failed_items() == (set(), {name}), rep.text(True)
