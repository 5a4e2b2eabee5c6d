"""GPU tests of the validation metrics (csrc/metrics.hip, metrics.py, pipeline.Evaluate, hdr_io.write_preview) against the float64
reference tests/metrics_ref.py.

Bars: the pointwise metrics and the scales <= 1e-5 relative (the project's per-layer bar: double-accumulated fp32 terms, each formed
to a few ulp of itself), peak exact, ssim_mu <= 1e-5 absolute (fp32 moments about a per-tile shift stay within 3e-8 of float64 on
the CPU; raw moments lose up to 3.8e-6)."""
import functools
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from conftest import GOLDEN, quantised_image
from oracle import nets

pytestmark = pytest.mark.gpu

TH, TW = 16, 32                  # asserted against K.METRICS_TILE below: the shapes are built from the kernel's tile
SHAPES = [(3, 11, 11), (3, 11, TW + 10), (3, 12, 13), (3, 27, 43), (3, TH + 10, TW + 10), (3, TH + 11, TW + 10),
          (3, 2 * TH + 9, 2 * TW + 11), (4, 256, 256)]
LAWS = ["quantised", "flat", "ramp", "clamps"]
POINTWISE = ("mse_l", "mse_mu", "l1_logc", "scale_pred", "scale_gt")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(shape, law):
    """(pred, gt) float32 [N, H, W, 3]; the images of a batch have different means and peaks"""
    n, h, w = shape
    rng = np.random.default_rng(1000 * h + w + 7 * LAWS.index(law))
    full = (n, h, w, 3)
    if law == "quantised":                                       # SURVEY.md 8d input law times a highlight boost
        gt = quantised_image(rng, full) * rng.uniform(1.0, 4.0, full)
        pred = gt * (1.0 + 0.05 * rng.standard_normal(full))
    elif law == "flat":
        gt = 0.9 + 1e-3 * rng.standard_normal(full)
        pred = gt + 1e-3 * rng.standard_normal(full)
    elif law == "ramp":
        gt = np.broadcast_to((0.1 + 0.8 * np.arange(w) / (w - 1.0))[None, None, :, None], full) + 2e-3 * rng.standard_normal(full)
        pred = gt + 2e-3 * rng.standard_normal(full)
    else:                                                        # both clamps: exact zeros, and values above the gt's maximum
        gt = quantised_image(rng, full) * rng.uniform(1.0, 4.0, full)
        pred = gt * (1.0 + 0.05 * rng.standard_normal(full))
        u = rng.random(full)
        pred = np.where(u < 0.10, 0.0, pred)
        pred = np.where(u > 0.95, gt.max(axis=(1, 2, 3), keepdims=True) * rng.uniform(1.01, 3.0, full), pred)
    gain = np.array([1.0, 2.5, 0.4, 1.7])[:n, None, None, None]
    pred, gt = (pred * gain).astype(np.float32), (gt * gain).astype(np.float32)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def reference(shape, law, normalise):
    pred, gt = inputs(shape, law)
    return R.hdr_metrics(pred, gt, normalise)


def check(got, ref, label):
    got = {k: host(v) for k, v in got.items()}
    for k in got:
        assert got[k].dtype == np.float64 and got[k].shape == ref[k].shape, k
    fig = {k: float(np.abs(got[k] / ref[k] - 1.0).max()) for k in POINTWISE}
    fig["ssim_mu"] = float(np.abs(got["ssim_mu"] - ref["ssim_mu"]).max())
    print(label, " ".join("%s=%.2e" % kv for kv in fig.items()), "peak_equal=%s" % np.array_equal(got["peak"], ref["peak"]))
    for k in POINTWISE:
        assert fig[k] <= 1e-5, (k, fig[k], got[k], ref[k])
    assert np.array_equal(got["peak"], ref["peak"]), (got["peak"], ref["peak"])
    assert fig["ssim_mu"] <= 1e-5, (got["ssim_mu"], ref["ssim_mu"])


def test_tile_constant(shdr):
    assert shdr._ops.METRICS_TILE == (TH, TW)


@pytest.mark.parametrize("normalise", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_metrics_match_reference(shdr, shape, law, normalise):
    pred, gt = inputs(shape, law)
    ref = reference(shape, law, normalise)
    assert len(set(gt.max(axis=(1, 2, 3)))) == shape[0] == len(set(np.round(gt.mean(axis=(1, 2, 3)), 3)))    # per-image indexing shows
    got = shdr._ops.hdr_metrics(dev(pred), dev(gt), normalise=normalise)
    check(got, ref, "%s %s normalise=%s" % (shape, law, normalise))


def test_bit_reproducible(shdr):
    pred, gt = (dev(a) for a in inputs((4, 256, 256), "quantised"))
    a = shdr._ops.hdr_metrics(pred, gt)
    b = shdr._ops.hdr_metrics(pred, gt)
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].dtype == torch.float64, k


def test_stream_ordered(shdr):
    """on a side stream, fed by work queued on that stream just before: the two launches and their workspace follow the stream"""
    shape = (3, 2 * TH + 9, 2 * TW + 11)
    pred, gt = inputs(shape, "quantised")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p = dev(pred * 0.5) * 2.0                                # exact in fp32: the same values, produced on the side stream
        g = dev(gt * 0.5) * 2.0
        got = shdr._ops.hdr_metrics(p, g, normalise=True)
    side.synchronize()
    check(got, reference(shape, "quantised", True), "side stream")


def test_l1_logc_is_the_finetuning_loss(shdr):
    K = shdr._ops
    pred, gt = inputs((4, 256, 256), "quantised")
    gt = gt * (0.5 / gt.astype(np.float64).mean(axis=(1, 2, 3), keepdims=True)).astype(np.float32)       # gt at mean 0.5
    p, g = dev(pred), dev(gt)
    got = K.hdr_metrics(p, g, normalise=True)
    assert np.abs(host(got["scale_gt"]) - 1.0).max() <= 1e-5
    loss = host(K.diff_loss(K.logc(K.mean_norm(p, 1e-6, 0.5)), K.logc(g), 1)).astype(np.float64)
    fig = np.abs(host(got["l1_logc"]) / loss - 1.0).max()
    print("l1_logc vs diff_loss(logc(mean_norm)):", fig)
    assert fig <= 1e-5


def test_functional_form_adds_psnr(shdr):
    shape = (3, 27, 43)
    pred, gt = inputs(shape, "quantised")
    m = shdr.metrics.hdr_metrics(dev(pred), dev(gt))
    ref = reference(shape, "quantised", True)
    assert np.abs(host(m["psnr_l"]) + 10 * np.log10(ref["mse_l"])).max() <= 1e-4           # 1e-5 relative in mse = 4.3e-5 dB
    assert np.abs(host(m["psnr_mu"]) + 10 * np.log10(ref["mse_mu"])).max() <= 1e-4
    assert set(m) == {"mse_l", "mse_mu", "l1_logc", "ssim_mu", "peak", "scale_pred", "scale_gt", "psnr_l", "psnr_mu"}


def test_evaluator_accumulates(shdr):
    M = shdr.metrics
    pred, gt = (dev(a) for a in inputs((4, 256, 256), "quantised"))
    one, four = M.Evaluator(), M.Evaluator()
    four.update(pred, gt)
    for i in range(4):
        one.update(pred[i:i + 1], gt[i:i + 1])
    a, b = one.result(), four.result()
    assert a["images"] == 4 == b["images"]
    assert set(a) == {"images", "psnr_l", "psnr_mu", "ssim_mu", "l1_logc", "psnr_l_min", "psnr_mu_min"}
    for k in a:
        assert abs(a[k] - b[k]) <= 1e-12 * max(1.0, abs(b[k])), k
    m = M.hdr_metrics(pred, gt)
    assert b["psnr_mu"] == pytest.approx(float(m["psnr_mu"].mean()), rel=1e-12)
    assert b["psnr_l_min"] == float(m["psnr_l"].min()) and b["ssim_mu"] == pytest.approx(float(m["ssim_mu"].mean()), rel=1e-12)
    assert one.state.dtype == torch.float64 and one.state.is_cuda and one.state.numel() == 7


def _nets(shdr, g):
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    return [getattr(shdr, mods[k]).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), int(g["seed_" + k])))
            for k in ("deq", "lin", "hal", "ref")]


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_pipeline_evaluate(shdr, precision):
    g = np.load(os.path.join(GOLDEN, "inference_64.npz"))
    run = shdr.pipeline.Inference(*_nets(shdr, g), precision=precision)
    ldr = dev(g["ldr"])
    rng = np.random.default_rng(5)
    gt = dev(np.abs(g["hdr"]) * (1.0 + 0.1 * rng.standard_normal(g["hdr"].shape)) + 1e-3)      # a synthetic ground truth
    direct = run(ldr)
    ev = shdr.pipeline.Evaluate(run)
    out = ev(ldr, gt)
    assert torch.equal(out, direct)
    res = ev.evaluator.result()
    m = shdr.metrics.hdr_metrics(direct, gt)
    assert res["images"] == ldr.shape[0]
    for k in ("psnr_l", "psnr_mu", "ssim_mu", "l1_logc"):
        assert res[k] == pytest.approx(float(m[k].mean()), rel=1e-12), k
        assert np.isfinite(res[k]), k
    again = shdr.pipeline.Evaluate(run).run([(ldr, gt), (ldr, gt)])
    assert again["images"] == 2 * ldr.shape[0] and again["psnr_mu"] == pytest.approx(res["psnr_mu"], rel=1e-12)


def test_tonemap_u8(shdr):
    K = shdr._ops
    rng = np.random.default_rng(6)
    x = (quantised_image(rng, (12, 13, 3)) * rng.uniform(1.0, 4.0, (12, 13, 3))).astype(np.float32)
    x[3, 4] = 0.0
    ref = R.tonemap_u8(x)
    got = host(K.tonemap_u8(dev(x)))
    assert got.dtype == np.uint8 and got.shape == ref.shape
    diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    print("tonemap_u8: max code difference %d, equal on %.4f" % (diff.max(), (diff == 0).mean()))
    assert diff.max() <= 1 and (diff == 0).mean() >= 0.99
    assert (got[x == x.max()] == 255).all() and (got[x == 0.0] == 0).all() and (x == 0.0).sum() >= 3
    assert np.array_equal(host(K.tonemap_u8(dev(x), reverse_channels=True)), got[..., ::-1])
    # an explicit peak, and a batch with one peak per image
    peak = torch.tensor([2.0, 3.0], device="cuda", dtype=torch.float64)
    xb = np.stack([x, 0.5 * x])
    gb = host(K.tonemap_u8(dev(xb), peak=peak))
    for i in range(2):
        d = np.abs(gb[i].astype(np.int32) - R.tonemap_u8(xb[i], peak=float(peak[i])).astype(np.int32))
        assert d.max() <= 1 and (d == 0).mean() >= 0.99


def test_write_preview_round_trips(shdr, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(8)
    x = dev(quantised_image(rng, (21, 34, 3)) * 3.0)
    path = str(tmp_path / "preview.png")
    shdr.hdr_io.write_preview(path, x)
    with Image.open(path) as im:
        back = np.array(im)
    assert np.array_equal(back, host(shdr._ops.tonemap_u8(x)))
    shdr.hdr_io.write_preview(path, x, reverse_channels=True)
    with Image.open(path) as im:
        assert np.array_equal(np.array(im), back[..., ::-1])
