"""HDR-Real folder reader on the device (singlehdr-tf2_amd/hdr_real.py, csrc/hdr_real.hip) against the NumPy restatement of
hdr_real_ref.py and against the record route (write_tfrecords -> tfrecord.HdrRealDataset).

Shapes are the smallest that reach each branch: patch sizes 16 and 24 (one partial 32 x 32 tile), 40 (a full tile plus partial
ones) and one 256 case; strides 4 and 8; images 40 x 52, 33 x 47 and 24 x 24, whose odd widths and border offsets make the uint8
rows start at every byte alignment.  HDR values are RGBE-decoded with exponents in a 16-wide range, so every sum of them is exact
in float64 whatever its order, and the statistics and the gather are held to bit equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import exr_ref as X
import hdr_real_ref as R
from conftest import rel_err
from oracle import nets

pytestmark = pytest.mark.gpu

SHAPES = [(40, 52), (33, 47), (24, 24)]


def rgbe_bytes(rng, h, w, lo=120, hi=136):
    """random RGBE pixels with exponents in [lo, hi): values k * 2^(e - 136), k < 256"""
    p = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    p[..., 3] = rng.integers(lo, hi, (h, w), dtype=np.uint8)
    return p


def pair(rng, h, w, shdr):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), shdr.hdr_io.rgbe_decode(rgbe_bytes(rng, h, w))


@pytest.fixture(scope="module")
def data(shdr):
    rng = np.random.default_rng(7)
    ldr, hdr = zip(*[pair(rng, h, w, shdr) for h, w in SHAPES])
    return list(ldr), list(hdr)


@pytest.fixture(scope="module")
def folder16(shdr, data):
    return shdr.hdr_real.HdrRealFolder.from_arrays(*data, size=16, stride=4, seed=3)


def ref_stats(folder, ldr, hdr):
    out = [R.patch_stats(R.crop(ldr[f], h1, w1, folder.size), R.crop(hdr[f], h1, w1, folder.size)) for f, h1, w1 in folder.candidates]
    return np.array([c for c, _ in out], dtype=np.int32), np.array([m for _, m in out], dtype=np.float32)


def ref_render(folder, ldr, hdr, params):
    kept_means = folder.means[folder.keep]
    outs = []
    for p, flip, rot in np.asarray(params):
        f, h1, w1 = folder.patches[p]
        outs.append(R.render(R.crop(ldr[f], h1, w1, folder.size), R.crop(hdr[f], h1, w1, folder.size), kept_means[p], flip, rot))
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def host(t):
    return t.cpu().numpy()


# --- statistics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,stride", [(16, 4), (24, 8), (40, 8)])
def test_statistics_bit_exact(shdr, data, size, stride):
    ldr, hdr = data
    folder = shdr.hdr_real.HdrRealFolder.from_arrays(ldr, hdr, size=size, stride=stride)
    want = [(f, h1, w1) for f, (h, w) in enumerate(SHAPES) for h1, w1 in shdr.hdr_real.enumerate_patches(h, w, size, stride)]
    assert folder.candidates == want and len(want) > 0
    count, mean = ref_stats(folder, ldr, hdr)
    assert np.array_equal(folder.extreme_counts, count) and folder.extreme_counts.dtype == np.int32
    assert same_bits(folder.means, mean)
    assert np.array_equal(folder.keep, count <= size * size // 2)
    assert folder.patches == [c for c, k in zip(want, folder.keep) if k]


def test_statistics_at_the_tie_values_and_the_keep_threshold(shdr):
    """one 16 x 16 patch per image: exactly 128 extreme pixels (kept), 129 (dropped), all-249, all-6, and mixtures of 248 / 249 /
    250 / 5 / 6 / 7, grey (one value per pixel) and coloured (one per channel)"""
    rng = np.random.default_rng(11)
    ties = np.array([248, 249, 250, 5, 6, 7], dtype=np.uint8)

    def half_extreme(n):
        img = np.full((256, 3), 128, dtype=np.uint8)
        img[rng.permutation(256)[:n]] = np.where(rng.random((n, 1)) < 0.5, 255, 0).astype(np.uint8)
        return img.reshape(16, 16, 3)
    grey = np.repeat(ties[rng.integers(0, 6, (16, 16, 1))], 3, axis=2)
    ldr = [half_extreme(128), half_extreme(129), np.full((16, 16, 3), 249, np.uint8), np.full((16, 16, 3), 6, np.uint8), grey,
           ties[rng.integers(0, 6, (16, 16, 3))]]
    hdr = [shdr.hdr_io.rgbe_decode(rgbe_bytes(rng, 16, 16)) for _ in ldr]
    folder = shdr.hdr_real.HdrRealFolder.from_arrays(ldr, hdr, size=16, stride=4)
    assert folder.candidates == [(f, 0, 0) for f in range(6)]
    count, mean = ref_stats(folder, ldr, hdr)
    print("extreme counts at the tie values:", folder.extreme_counts.tolist())
    assert np.array_equal(folder.extreme_counts, count) and same_bits(folder.means, mean)
    assert folder.extreme_counts[0] == 128 and folder.extreme_counts[1] == 129
    assert folder.keep[0] and not folder.keep[1]
    assert (0, 0, 0) in folder.patches and (1, 0, 0) not in folder.patches
    assert folder.patches == [(f, 0, 0) for f in range(6) if count[f] <= 128]


# --- gather ------------------------------------------------------------------------------------------------------------
def corner_patches(folder, f):
    h, w = folder.shapes[f]
    s = folder.size
    return [folder.patches.index((f, h1, w1)) for h1 in (0, h - s) for w1 in (0, w - s)]


def test_gather_every_flip_and_rot_bit_exact(shdr, data, folder16):
    ldr, hdr = data
    assert folder16.keep.all()                                   # random LDR: nothing is filtered, indices are candidates'
    picks = corner_patches(folder16, 0) + corner_patches(folder16, 1) + [len(folder16.patches) - 1, 37, 101]
    params = np.array([(p, flip, rot) for i, p in enumerate(picks) for flip in (0, 1) for rot in range(5)
                       if i < 2 or (flip + rot + i) % 3 == 0], dtype=np.int32)        # two patches get all ten, the others a third
    assert {(f, r) for _, f, r in params[:10].tolist()} == {(f, r) for f in (0, 1) for r in range(5)}
    assert len({folder16.patches[p][0] for p in params[:, 0]}) == 3                   # one batch over images of three sizes
    got_l, got_h = folder16.render(params)
    want_l, want_h = ref_render(folder16, ldr, hdr, params)
    assert got_l.dtype == got_h.dtype == torch.float32 and tuple(got_l.shape) == (len(params), 16, 16, 3)
    assert same_bits(host(got_l), want_l) and same_bits(host(got_h), want_h)


@pytest.mark.parametrize("size,stride", [(24, 8), (40, 8)])
def test_gather_partial_and_multiple_tiles_bit_exact(shdr, data, size, stride):
    ldr, hdr = data
    folder = shdr.hdr_real.HdrRealFolder.from_arrays(ldr, hdr, size=size, stride=stride)
    n = len(folder.patches)
    params = np.array([((3 * k) % n, flip, rot) for k, (flip, rot) in enumerate((f, r) for f in (0, 1) for r in range(5))], dtype=np.int32)
    got_l, got_h = folder.render(params)
    want_l, want_h = ref_render(folder, ldr, hdr, params)
    assert same_bits(host(got_l), want_l) and same_bits(host(got_h), want_h)


def test_gather_batch_of_one(shdr, data, folder16):
    ldr, hdr = data
    params = np.array([[corner_patches(folder16, 1)[3], 1, 3]], dtype=np.int32)
    got_l, got_h = folder16.render(params)
    want_l, want_h = ref_render(folder16, ldr, hdr, params)
    assert tuple(got_l.shape) == (1, 16, 16, 3) and same_bits(host(got_l), want_l) and same_bits(host(got_h), want_h)


def test_real_geometry_once(shdr):
    """size 256, stride 64 on one 320 x 512 pair: 10 grid patches and the duplicated border row"""
    rng = np.random.default_rng(5)
    l, h = pair(rng, 320, 512, shdr)
    l[:200, :300] = 255                                          # the top-left patches are mostly white: filtered
    folder = shdr.hdr_real.HdrRealFolder.from_arrays([l], [h])
    grid = [(0, h1, w1) for h1 in (0, 64) for w1 in (0, 64, 128, 192, 256)]
    assert folder.candidates == grid + [(0, 64, w1) for w1 in (0, 64, 128, 192, 256)]
    count, mean = ref_stats(folder, [l], [h])
    assert np.array_equal(folder.extreme_counts, count) and same_bits(folder.means, mean)
    assert not folder.keep.all() and folder.keep.any()
    n = len(folder.patches)
    params = np.array([(k % n, flip, rot) for k, (flip, rot) in enumerate((f, r) for f in (0, 1) for r in range(5))], dtype=np.int32)
    got_l, got_h = folder.render(params)
    want_l, want_h = ref_render(folder, [l], [h], params)
    assert same_bits(host(got_l), want_l) and same_bits(host(got_h), want_h)


# --- against the record route ------------------------------------------------------------------------------------------
def test_matches_the_record_route_end_to_end(shdr, data, folder16, tmp_path):
    out_dir = str(tmp_path / "records")
    paths = shdr.hdr_real.write_tfrecords(folder16, out_dir)
    n = len(folder16.patches)
    assert len(set(folder16.patches)) < n                        # the reference's duplicates are written
    assert len(paths) == -(-n // 32) and os.path.basename(paths[0]) == "train_4_0000.tfrecords"
    records = shdr.tfrecord.HdrRealDataset(out_dir, augment=False, shuffle_buffer=1, imshape=(16, 16, 3))
    batches = list(records)
    assert len(batches) == -(-n // 4) and n % 4 != 0 and batches[-1][0].shape[0] == n % 4
    worst = 0.0
    for k, (rec_l, rec_h) in enumerate(batches):
        idx = np.arange(4 * k, min(4 * k + 4, n))
        got_l, got_h = folder16.render(np.stack([idx, 0 * idx, 0 * idx], 1))
        assert same_bits(host(got_l), host(rec_l))
        worst = max(worst, rel_err(host(got_h), host(rec_h)))
    print("largest relative HDR difference between the folder and the record route: %.3g" % worst)
    assert worst <= 1e-4


# --- epochs ------------------------------------------------------------------------------------------------------------
def test_epoch_over_three_ranks_visits_every_patch_once(shdr, data):
    ranks = [shdr.hdr_real.HdrRealFolder.from_arrays(*data, size=16, stride=4, seed=9, rank=r, world_size=3, batch_size=5) for r in range(3)]
    n = len(ranks[0].patches)
    seen = []
    for r, folder in enumerate(ranks):
        epoch = folder.epoch()
        assert len(epoch) == len(folder) == -(-len(range(r, n, 3)) // 5)
        assert all(len(p) == 5 for p in epoch[:-1]) and 0 < len(epoch[-1]) <= 5
        seen += [int(p) for batch in epoch for p in batch[:, 0]]
    assert sorted(seen) == list(range(n))


def test_same_seed_same_epoch_other_seed_another(shdr, data):
    def epoch(seed):
        return np.concatenate(shdr.hdr_real.HdrRealFolder.from_arrays(*data, size=16, stride=4, seed=seed).epoch())
    a, b, c = epoch(1), epoch(1), epoch(2)
    assert np.array_equal(a, b) and not np.array_equal(a[:, 0], c[:, 0])
    assert set(a[:, 1].tolist()) == {0, 1} and set(a[:, 2].tolist()) == {0, 1, 2, 3, 4}          # rot 4 occurs


def test_no_augmentation_renders_the_patches_as_they_are(shdr, data):
    ldr, hdr = data
    folder = shdr.hdr_real.HdrRealFolder.from_arrays(ldr, hdr, size=16, stride=4, seed=4, augment=False, batch_size=6)
    epoch = folder.epoch()
    assert all((p[:, 1:] == 0).all() for p in epoch)
    folder2 = shdr.hdr_real.HdrRealFolder.from_arrays(ldr, hdr, size=16, stride=4, seed=4, augment=False, batch_size=6)
    got_l, got_h = next(iter(folder2))
    want_l, want_h = ref_render(folder2, ldr, hdr, epoch[0])
    assert same_bits(host(got_l), want_l) and same_bits(host(got_h), want_h)
    assert np.array_equal(folder.draw(3)[:, 1:], np.zeros((3, 2), dtype=np.int32))


# --- determinism -------------------------------------------------------------------------------------------------------
def test_two_launches_give_the_same_bits(shdr, folder16):
    K = shdr._ops
    cand = np.asarray(folder16.candidates, dtype=np.int32)
    cand_dev = torch.from_numpy(cand).cuda()
    images_dev = torch.from_numpy(folder16.images).cuda()
    runs = [K.pair_patch_stats(folder16.ldr_arena, folder16.hdr_arena, folder16.images, images_dev, cand, cand_dev, 16) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and same_bits(host(runs[0][1]), host(runs[1][1]))
    assert np.array_equal(host(runs[0][0]), folder16.extreme_counts) and same_bits(host(runs[0][1]), folder16.means)
    params = folder16.draw(7)
    a, b = folder16.render(params), folder16.render(params)
    assert same_bits(host(a[0]), host(b[0])) and same_bits(host(a[1]), host(b[1]))


# --- refusals: the host tables are checked before anything is launched ---------------------------------------------------
@pytest.fixture(scope="module")
def tables(shdr):
    """one 20 x 24 pair and two good 16 x 16 patches"""
    rng = np.random.default_rng(2)
    l, h = pair(rng, 20, 24, shdr)
    return dict(ldr=torch.from_numpy(l.reshape(-1)).cuda(), hdr=torch.from_numpy(h.reshape(-1)).cuda(),
                images=np.array([[0, 20, 24]], dtype=np.int64), patches=np.array([[0, 0, 0], [0, 4, 8]], dtype=np.int32),
                mean=torch.ones(2, device="cuda"), samples=np.array([[0, 0, 0], [1, 1, 4]], dtype=np.int32))


def call_stats(shdr, t, size=16, **over):
    t = dict(t, **over)
    return shdr._ops.pair_patch_stats(t["ldr"], t["hdr"], t["images"], torch.from_numpy(t["images"]).cuda(), t["patches"],
                                      torch.from_numpy(t["patches"]).cuda(), size)


def call_gather(shdr, t, size=16, **over):
    t = dict(t, **over)
    return shdr._ops.pair_patch_gather(t["ldr"], t["hdr"], t["images"], torch.from_numpy(t["images"]).cuda(), t["patches"],
                                       torch.from_numpy(t["patches"]).cuda(), t["mean"], t["samples"], size)


def test_good_tables_are_accepted(shdr, tables):
    count, mean = call_stats(shdr, tables)
    assert count.shape == (2,) and mean.shape == (2,)
    assert call_gather(shdr, tables)[0].shape == (2, 16, 16, 3)


def test_refuses_null_pointers(shdr, tables):
    lib = shdr._lib.load()
    t = tables
    vp = ctypes.c_void_p
    img_d, pat_d, smp_d = (torch.from_numpy(t[k]).cuda() for k in ("images", "patches", "samples"))
    count, mean = torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(2, device="cuda")
    out = torch.empty((2, 16, 16, 3), device="cuda")
    good_s = [vp(t["ldr"].data_ptr()), vp(t["hdr"].data_ptr()), 480, vp(t["images"].ctypes.data), vp(img_d.data_ptr()), 1,
              vp(t["patches"].ctypes.data), vp(pat_d.data_ptr()), 2, 16, vp(count.data_ptr()), vp(mean.data_ptr()), None]
    for k in (0, 1, 3, 4, 6, 7, 10, 11):
        args = list(good_s)
        args[k] = None
        assert lib.shdr_pair_patch_stats(*args) == -5 and b"null" in lib.shdr_last_error()
    out2 = torch.empty_like(out)
    good_g = good_s[:9] + [vp(t["mean"].data_ptr()), vp(t["samples"].ctypes.data), vp(smp_d.data_ptr()), 2, 16, vp(out.data_ptr()),
                           vp(out2.data_ptr()), None]
    for k in (0, 1, 3, 4, 6, 7, 9, 10, 11, 14, 15):
        args = list(good_g)
        args[k] = None
        assert lib.shdr_pair_patch_gather_f32(*args) == -5 and b"null" in lib.shdr_last_error()


@pytest.mark.parametrize("call", [call_stats, call_gather])
def test_refuses_non_positive_size(shdr, tables, call):
    for size in (0, -16):
        with pytest.raises(RuntimeError, match="size"):
            call(shdr, tables, size=size)


@pytest.mark.parametrize("call", [call_stats, call_gather])
def test_refuses_a_patch_that_leaves_its_image(shdr, tables, call):
    for bad in ([0, 5, 0], [0, 0, 9], [0, -1, 0], [0, 0, -1]):
        with pytest.raises(RuntimeError, match="leaves its"):
            call(shdr, tables, patches=np.array([bad, [0, 4, 8]], dtype=np.int32))
    with pytest.raises(RuntimeError, match="leaves the arenas"):                      # an image that leaves the arenas
        call(shdr, tables, images=np.array([[1, 20, 24]], dtype=np.int64))
    with pytest.raises(RuntimeError, match="leaves its"):                             # size 21: no patch fits the 20 rows
        call(shdr, tables, size=21)


@pytest.mark.parametrize("call", [call_stats, call_gather])
def test_refuses_an_image_index_out_of_the_table(shdr, tables, call):
    for img in (1, -1):
        with pytest.raises(RuntimeError, match="names image"):
            call(shdr, tables, patches=np.array([[img, 0, 0], [0, 4, 8]], dtype=np.int32))


def test_refuses_a_patch_index_out_of_the_table(shdr, tables):
    for p in (2, -1):
        with pytest.raises(RuntimeError, match="names patch"):
            call_gather(shdr, tables, samples=np.array([[p, 0, 0]], dtype=np.int32))


def test_refuses_rot_and_flip_out_of_range(shdr, tables):
    for rot in (5, -1):
        with pytest.raises(RuntimeError, match="rot"):
            call_gather(shdr, tables, samples=np.array([[0, 0, 0], [1, 0, rot]], dtype=np.int32))
    with pytest.raises(RuntimeError, match="flip"):
        call_gather(shdr, tables, samples=np.array([[0, 2, 0]], dtype=np.int32))


def test_refuses_an_empty_batch(shdr, tables):
    with pytest.raises(RuntimeError, match="batch"):
        call_gather(shdr, tables, samples=np.zeros((0, 3), dtype=np.int32))


# --- files -------------------------------------------------------------------------------------------------------------
def write_pair_files(shdr, root, name, rgbe, ldr_u8):
    from PIL import Image
    os.makedirs(os.path.join(root, "HDR_gt"), exist_ok=True)
    os.makedirs(os.path.join(root, "LDR_in"), exist_ok=True)
    shdr.hdr_io.write_hdr(os.path.join(root, "HDR_gt", name + ".hdr"), rgbe)
    Image.fromarray(ldr_u8).save(os.path.join(root, "LDR_in", name + ".jpg"), quality=92)


def test_a_folder_of_two_pairs_loads(shdr, tmp_path):
    rng = np.random.default_rng(21)
    root = str(tmp_path)
    rgbe = {}
    for name, (h, w) in (("b_scene", (33, 47)), ("a_scene", (40, 52))):
        rgbe[name] = rgbe_bytes(rng, h, w)
        write_pair_files(shdr, root, name, rgbe[name], rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    folder = shdr.hdr_real.HdrRealFolder(root, size=16, stride=8)
    assert [os.path.basename(h) for h, _ in folder.files] == ["a_scene.hdr", "b_scene.hdr"]           # sorted, paired by position
    assert folder.shapes == [(40, 52), (33, 47)]
    ldr, hdr = [], []
    for i, name in enumerate(("a_scene", "b_scene")):
        l, h = folder.host_pair(i)
        assert l.dtype == np.uint8 and same_bits(l, shdr.hdr_io.read_ldr(os.path.join(root, "LDR_in", name + ".jpg")))
        assert same_bits(h, shdr.hdr_io.rgbe_decode(rgbe[name]))                                      # RGB, as the records hold it
        ldr.append(l)
        hdr.append(h)
    count, mean = ref_stats(folder, ldr, hdr)
    assert np.array_equal(folder.extreme_counts, count) and same_bits(folder.means, mean)
    ref_l, ref_h = next(iter(folder))
    assert tuple(ref_l.shape) == tuple(ref_h.shape) == (4, 16, 16, 3)


def test_count_mismatch_names_the_files(shdr, tmp_path):
    rng = np.random.default_rng(22)
    root = str(tmp_path)
    write_pair_files(shdr, root, "one", rgbe_bytes(rng, 16, 16), rng.integers(0, 256, (16, 16, 3), dtype=np.uint8))
    shdr.hdr_io.write_hdr(os.path.join(root, "HDR_gt", "two.hdr"), rgbe_bytes(rng, 16, 16))
    with pytest.raises(ValueError, match=r"two\.hdr") as exc:
        shdr.hdr_real.HdrRealFolder(root, size=16, stride=4)
    assert "one.jpg" in str(exc.value)


def test_size_mismatch_names_the_files(shdr, tmp_path):
    rng = np.random.default_rng(23)
    root = str(tmp_path)
    write_pair_files(shdr, root, "ok", rgbe_bytes(rng, 16, 16), rng.integers(0, 256, (16, 16, 3), dtype=np.uint8))
    write_pair_files(shdr, root, "odd", rgbe_bytes(rng, 16, 20), rng.integers(0, 256, (20, 16, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"odd\.hdr.*16 x 20.*odd\.jpg.*20 x 16"):
        shdr.hdr_real.HdrRealFolder(root, size=16, stride=4)


def test_exr_ground_truth_gives_the_arena_of_its_radiance_copy(shdr, tmp_path):
    """the same half-representable values (8-bit mantissas, exponents 2^-8 .. 2^-1 per unit) as ZIP HALF OpenEXR and as Radiance"""
    from PIL import Image
    rng = np.random.default_rng(24)
    rgbe = rgbe_bytes(rng, 33, 47, 128, 136)
    values = shdr.hdr_io.rgbe_decode(rgbe)
    assert np.array_equal(values.astype(np.float16).astype(np.float32), values)
    ldr = rng.integers(0, 256, (33, 47, 3), dtype=np.uint8)
    rad, ex = str(tmp_path / "rad"), str(tmp_path / "exr")
    write_pair_files(shdr, rad, "s", rgbe, ldr)
    os.makedirs(os.path.join(ex, "HDR_gt"))
    os.makedirs(os.path.join(ex, "LDR_in"))
    X.write_exr(os.path.join(ex, "HDR_gt", "s.exr"), {c: (values[..., k], X.HALF) for k, c in enumerate("RGB")}, X.ZIP)
    Image.fromarray(ldr).save(os.path.join(ex, "LDR_in", "s.jpg"), quality=92)
    a = shdr.hdr_real.HdrRealFolder(rad, size=16, stride=8)
    b = shdr.hdr_real.HdrRealFolder(ex, size=16, stride=8)
    assert same_bits(host(b.hdr_arena), host(a.hdr_arena)) and same_bits(host(a.hdr_arena), values.reshape(-1))
    assert same_bits(host(b.ldr_arena), host(a.ldr_arena))
    assert b.patches == a.patches and same_bits(b.means, a.means)


# --- one fine-tuning step ----------------------------------------------------------------------------------------------
def test_a_rendered_batch_feeds_one_finetune_step(shdr):
    rng = np.random.default_rng(31)
    l, h = pair(rng, 64, 96, shdr)
    folder = shdr.hdr_real.HdrRealFolder.from_arrays([l], [h], size=64, stride=32, batch_size=2)
    ref_ldr, ref_hdr = folder.render(folder.draw())
    assert tuple(ref_ldr.shape) == (2, 64, 64, 3) and ref_ldr.dtype == ref_hdr.dtype == torch.float32
    mods = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")
    ms = {k: getattr(shdr, mod).model().load_numpy(nets.init_params(getattr(nets, k + "_spec")(), 95 + i))
          for i, (k, mod) in enumerate(mods.items())}
    step = shdr.pipeline.FinetuneStep(ms["deq"], ms["lin"], ms["hal"], ms["ref"], lr=1e-4)
    out = step(ref_ldr, ref_hdr, apply=False)
    loss = out["loss_sum"].detach()
    assert torch.isfinite(loss).all() and float(loss.sum()) > 0
    for net in ms.values():
        for t in net.trainable_variables:
            assert t.grad is not None and torch.isfinite(t.grad).all()
