"""GPU tests of the training-set reader (dataset.py of the reference) against the float32 restatement in dataset_ref.py:
the resident images, the crop means, the patch sampler for forced draws, and one reader -> camera -> joint step."""
import importlib
import os

import numpy as np
import pytest
import torch

import dataset_ref as R
from oracle import imageio as O
from oracle import nets
from test_dataset import write_dorf

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("singlehdr-tf2_amd")
D = pkg.dataset
IO = pkg.hdr_io

# (h, w): landscape, portrait, square; short side < 512 (upscale), = 512 (identity), about 1500 (downscale)
SHAPES = {"land.hdr": (600, 900), "port.hdr": (700, 520), "square.hdr": (512, 512), "small.hdr": (300, 400),
          "big.hdr": (1500, 2000), "bigsq.hdr": (1480, 1480)}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("hdr")
    rng = np.random.default_rng(20)
    for i, (name, (h, w)) in enumerate(sorted(SHAPES.items())):
        rgb = np.exp(rng.normal(0.0, 2.5, (h, w, 3))).astype(np.float32) * (1.0 + np.arange(3, dtype=np.float32))
        rgb[h // 3:h // 3 + 40, w // 4:w // 4 + 60] = 0.0                       # e == 0 pixels
        rgb[:7, :5] *= 1e4                                                        # bright corner
        IO.write_hdr(str(d / name), O.rgbe_encode(rgb))
    return str(d)


@pytest.fixture(scope="module")
def train_set(files):
    return D.PatchHDRDataset(files, sorted(SHAPES), True)


def _host(t):
    return t.detach().cpu().numpy()


def _check(got, want, tap, what):
    err = np.abs(got.astype(np.float64) - want)
    bad = err > 1e-6 * tap
    assert not bad.any(), "%s: %d values off, worst %g (tap %g)" % (what, bad.sum(), err[bad].max(), tap[bad][np.argmax(err[bad])])


def test_load_matches_restatement(files, train_set):
    for f, name in enumerate(sorted(SHAPES)):
        want, tap = R.load(IO.read_hdr(os.path.join(files, name)))
        got = _host(train_set.image(f))
        assert got.shape == want.shape and min(got.shape[:2]) == 512, name
        _check(got, want, tap, name)


def test_window_means(train_set):
    means = _host(train_set.means)
    for f in range(len(SHAPES)):
        img = _host(train_set.image(f))
        for p in (0, 1):
            ref = np.mean(R.window(img, p), dtype=np.float64)
            assert abs(means[2 * f + p] - ref) <= 1e-6 * ref, (f, p)
    again = D.PatchHDRDataset(os.path.dirname(train_set._hdr_dataset.path(0)), sorted(SHAPES), True)
    assert torch.equal(again.means, train_set.means) and torch.equal(again.arena, train_set.arena)       # deterministic


def _forced_params(n_patches):
    rows = []
    combos = [(256, 0, 0), (257, 0, 0), (512, 0, 0), (512, 255, 3), (700, 443, 100), (1024, 767, 767), (1024, 0, 767),
              (333, 76, 12)]
    for idx in range(n_patches):
        for c, (S, y0, x0) in enumerate(combos):
            k, f0, f1 = (idx + c) % 4, (idx + c) // 4 % 2, (idx + 3 * c) % 2
            rows.append([idx, S, y0, x0, k, f0, f1])
    for k in range(4):                                       # every k with every flip pair on one patch of each aspect
        for f0 in (0, 1):
            for f1 in (0, 1):
                for idx in (0, 3, 5, 8):
                    rows.append([idx, 1024, 767, 767, k, f0, f1])
    return np.array(rows, dtype=np.int32)


def test_sampler_matches_restatement(train_set):
    params = _forced_params(len(train_set))
    got = _host(train_set.render(params))
    assert got.shape == (len(params), 256, 256, 3)
    means = _host(train_set.means)
    imgs = [_host(train_set.image(f)) for f in range(len(SHAPES))]
    for n, (idx, S, y0, x0, k, f0, f1) in enumerate(params.tolist()):
        want, tap = R.patch(imgs[idx // 2], idx, S, y0, x0, k, f0, f1, means[idx])
        _check(got[n], want, tap, str(params[n].tolist()))


def test_getitem_and_invalid_params(train_set):
    x = train_set[3]
    assert tuple(x.shape) == (256, 256, 3) and torch.isfinite(x).all()
    for bad in ([len(train_set), 512, 0, 0, 0, 0, 0], [0, 255, 0, 0, 0, 0, 0], [0, 512, 257, 0, 0, 0, 0], [0, 512, 0, 0, 4, 0, 0]):
        with pytest.raises(ValueError):
            train_set.render(np.array([bad]))


def test_evaluation_crop(files):
    ev = D.PatchHDRDataset(files, sorted(SHAPES), False)
    params = D.draw_patch_params(np.arange(len(ev)), None, False)
    got = _host(ev.render(params))
    assert got.shape == (len(ev), 512, 512, 3)
    means = _host(ev.means)
    for idx in range(len(ev)):
        want, tap = R.patch(_host(ev.image(idx // 2)), idx, 512, 0, 0, 0, 0, 0, means[idx], is_training=False)
        _check(got[idx], want, tap, "eval %d" % idx)
    assert torch.equal(ev[5], ev.render(params[5:6])[0])


def _models():
    P = {k: nets.init_params(getattr(nets, k + "_spec")(), 80 + i) for i, k in enumerate(("deq", "lin", "hal"))}
    V = nets.init_params(nets.vgg_spec(), 83)
    dd = {n: [V[n + ".kernel"], V[n + ".bias"]] for n in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3")}
    return (pkg.dequantization_net.model().load_numpy(P["deq"]), pkg.linearization_net.model().load_numpy(P["lin"]),
            pkg.hallucination_net.model().load_numpy(P["hal"]), pkg.vgg16.Vgg16(data_dict=dd))


def test_reader_camera_joint_step(files, tmp_path):
    crf_path = str(tmp_path / "dorfCurves.txt")
    write_dorf(crf_path, n=201)
    ds = D.get_train_dataset(files, crf_path=crf_path)
    assert len(ds) == 2 * len(SHAPES) * 191 * 600
    item = ds[2 * len(SHAPES) * 191 * 5 + 2 * len(SHAPES) * 7 + 3]           # patch 3, CRF 7, t 5
    assert tuple(item[0].shape) == (256, 256, 3) and item[1].shape == (1024,) and item[3] == D.get_t_list(600)[5]
    a, b = D.RandDatasetReader(ds, 4, seed=7), D.RandDatasetReader(ds, 4, seed=7)
    for _ in range(3):
        ba, bb = a.read_batch_data(), b.read_batch_data()
        for x, y in zip(ba, bb):
            assert torch.equal(x, y)
    hdr, crf, invcrf, t = ba
    assert tuple(hdr.shape) == (4, 256, 256, 3) and tuple(crf.shape) == (4, 1024) and tuple(invcrf.shape) == (4, 1024)
    assert tuple(t.shape) == (4,)
    p = a.draw()
    hdr2, crf2, inv2, t2 = a.render(p)
    assert torch.equal(crf2.cpu(), torch.from_numpy(np.ascontiguousarray(ds.dataset_list[1].dataset_list[0][p[:, D.P_CRF]])))
    assert torch.equal(t2.cpu(), torch.from_numpy(D.get_t_list(600)[p[:, D.P_T]]))
    cam = pkg.camera.CameraPipeline(seed=3)
    batch = cam(hdr2, crf2, t2)
    deq, lin, hal, vgg = _models()
    step = pkg.pipeline.JointTrainStep(deq, lin, hal, vgg)
    out = step(batch, inv2)
    torch.cuda.synchronize()
    for k in ("loss_deq", "loss_lin", "loss_hal", "total"):
        assert torch.isfinite(out[k]).all(), k
