"""GPU tests of the gain-map kernels (csrc/gainmap.hip): K.gainmap_encode and K.gainmap_apply against their host twins BIT FOR BIT,
on every shape, factor and content case of gainmap_ref.py (the twins are held to the float64 reference by test_gainmap_host.py), with
guard bytes around every output and the workspace, and with descriptors that must be refused before anything is launched."""
import numpy as np
import pytest
import torch

import gainmap_ref as R

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guards_intact(K, info, names):
    g = info["guard"]
    assert g >= 64
    for name in names:
        raw = info[name].cpu().numpy()
        assert (raw[:g] == K.GAINMAP_GUARD).all() and (raw[-g:] == K.GAINMAP_GUARD).all(), name


def _encode_both(K, sdrs, hdrs, factors, scales, reverse, log2_range=(-4.0, 8.0)):
    images, _, _ = K.gainmap_images([s.shape[:2] for s in sdrs], factors)
    sdr = np.concatenate([s.reshape(-1, 3) for s in sdrs])
    hdr = np.concatenate([h.reshape(-1, 3) for h in hdrs])
    want_maps, want_meta = K.gainmap_encode_host(sdr, hdr, images, scales, log2_range, reverse)
    d_sdr, d_hdr = dev(sdr).reshape(-1), dev(hdr).reshape(-1)
    runs = []
    for _ in range(2):
        info = {}
        maps, meta = K.gainmap_encode(d_sdr, d_hdr, images, scales, log2_range, reverse, guard=64, info=info)
        torch.cuda.synchronize()
        _guards_intact(K, info, ("maps_raw", "meta_raw", "workspace_raw"))
        runs.append((maps.cpu().numpy(), meta.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])     # the same bits on a second run
    return runs[0][0], runs[0][1].view(K.GAINMAP_META_DTYPE), want_maps, want_meta


def _same_meta(got, want, what):
    for field in ("gain_min", "gain_max", "scale"):
        assert np.array_equal(got[field].view(np.uint32), want[field].view(np.uint32)), (what, field, got[field], want[field])
    assert np.array_equal(got["count"], want["count"]), (what, got["count"], want["count"])


@pytest.mark.parametrize("name", R.CONTENTS)
def test_encode_is_the_host_twin_bit_for_bit(shdr, name):
    K = shdr._ops
    for case in R.cases(name):
        maps, meta, want_maps, want_meta = _encode_both(K, [case["sdr"]], [case["hdr"]], case["factor"],
                                                        None if case["scale"] is None else [case["scale"]], case["reverse"])
        assert np.array_equal(maps, want_maps), (case["name"], int((maps != want_maps).sum()))
        _same_meta(meta, want_meta, case["name"])


@pytest.mark.parametrize("fixed", [False, True])
def test_mixed_batch_in_one_call(shdr, fixed):
    """all shapes and factors in a single call, contents mixed; more than one block of statistics and of cells in the largest image"""
    K = shdr._ops
    by_content = {name: R.cases(name) for name in R.CONTENTS}
    cases = [by_content[R.CONTENTS[i % len(R.CONTENTS)]][i] for i in range(len(R.SHAPES) * len(R.FACTORS))]
    extra = R.content("noise", (70, 200), 99)                       # 14000 pixels: 4 parts of statistics, 14 blocks of cells at factor 1
    sdrs = [c["sdr"] for c in cases] + [extra[0]]
    hdrs = [c["hdr"] if not c["reverse"] else c["hdr"][..., ::-1].copy() for c in cases] + [extra[1]]
    factors = [c["factor"] for c in cases] + [1]
    scales = [0.3 + 0.1 * i for i in range(len(sdrs))] if fixed else None
    maps, meta, want_maps, want_meta = _encode_both(K, sdrs, hdrs, factors, scales, False)
    assert np.array_equal(maps, want_maps)
    _same_meta(meta, want_meta, "batch")
    assert fixed or (want_meta["count"] > 0).any()
    maps, meta, want_maps, want_meta = _encode_both(K, sdrs, hdrs, factors, scales, True, (-1.0, 2.5))
    assert np.array_equal(maps, want_maps)
    _same_meta(meta, want_meta, "batch, reversed, narrow range")


def test_apply_is_the_host_twin_bit_for_bit(shdr):
    """every shape and factor; three- and one-channel maps, Gamma 1 / 2.2 / 0.8, other offsets, display_boost below (w = 0), inside and
    above (w = 1) the capacity range; then all of them in one launch"""
    K, U = shdr._ops, shdr.ultrahdr
    items, sdrs, maps = [], [], []
    for i, case in enumerate(R.cases("noise") + R.cases("specials")[-8:] + [dict(sdr=R.content("noise", (70, 200), 98)[0], hdr=R.content("noise", (70, 200), 98)[1],
                                                                                 factor=4, reverse=False, scale=None)]):
        images, _, _ = K.gainmap_images([case["sdr"].shape[:2]], case["factor"])
        codes, meta = K.gainmap_encode_host(case["sdr"].reshape(-1, 3), case["hdr"].reshape(-1, 3), images, reverse_channels=case["reverse"])
        mc = 3 if i % 3 else 1
        if mc == 1:
            codes = np.ascontiguousarray(codes.reshape(-1, 3)[:, 1])
        fields = U.metadata_of(meta[0])
        boost = (None, 0.5, 2.0 ** (fields["HDRCapacityMax"] * 0.37), 2.0 ** (fields["HDRCapacityMax"] + 1))[i % 4]
        H, W = case["sdr"].shape[:2]
        item = dict(height=H, width=W, factor=case["factor"], map_channels=mc, gain_min=meta[0]["gain_min"], gain_max=meta[0]["gain_max"],
                    gamma=(1.0, 2.2, 0.8)[i % 3], weight=U.weight_of(fields, boost))
        if i % 5 == 0:
            item.update(offset_sdr=0.03125, offset_hdr=0.0078125)
        items.append(item)
        sdrs.append(case["sdr"].reshape(-1, 3))
        maps.append(codes.reshape(-1))
    assert {it["weight"] for it in items} >= {0.0, 1.0} and any(0.0 < it["weight"] < 1.0 for it in items)
    for item, sdr, codes in list(zip(items, sdrs, maps)) + [(items, np.concatenate(sdrs), np.concatenate(maps))]:
        images, _ = K.gainmap_apply_images(item if isinstance(item, list) else [item])
        want = K.gainmap_apply_host(sdr, codes, images)
        info = {}
        got = K.gainmap_apply(dev(sdr), dev(codes), images, guard=64, info=info)
        torch.cuda.synchronize()
        _guards_intact(K, info, ("out_raw",))
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), item if not isinstance(item, list) else "batch"


def test_bad_descriptors_raise_before_any_launch(shdr):
    """an image outside its arena, factor 3, size 0, stale derived fields: ValueError from the host-side checks; the destinations that a
    launch would have written keep their guard pattern"""
    K = shdr._ops
    sdr, hdr = dev(np.zeros((64, 3), np.uint8)).reshape(-1), dev(np.zeros((64, 3), np.float32)).reshape(-1)
    good, _, _ = K.gainmap_images([(8, 8)], 4)
    for change, match in ((dict(pix_off=1), "leaves the arenas"), (dict(factor=3), "factor 3"), (dict(height=0), "0 x 8"),
                          (dict(width=0), "8 x 0"), (dict(cell_block0=1), "derived fields"), (dict(pix_off=-1), "leaves the arenas")):
        bad = good.copy()
        for k, v in change.items():
            bad[k] = v
        with pytest.raises(ValueError, match=match):
            K.gainmap_encode(sdr, hdr, bad)
    with pytest.raises(ValueError, match="scale"):
        K.gainmap_encode(sdr, hdr, good, [float("nan")])
    with pytest.raises(ValueError, match="range"):
        K.gainmap_encode(sdr, hdr, good, log2_range=(1.0, float("inf")))
    ap, _ = K.gainmap_apply_images([dict(height=8, width=8, factor=4, map_channels=3, gain_min=0.0, gain_max=1.0)])
    maps = dev(np.zeros(12, np.uint8))
    for change, match in ((dict(pix_off=1), "leaves the arena"), (dict(map_off=1), "map bytes"), (dict(block0=3), "block0"),
                          (dict(map_channels=2), "1 or 3 channels"), (dict(gamma=0.0), "gamma"), (dict(weight=1.5), "weight"),
                          (dict(factor=0), "factor 0"), (dict(map_width=3), "map is not that")):
        bad = ap.copy()
        for k, v in change.items():
            bad[k] = v
        with pytest.raises(ValueError, match=match):
            K.gainmap_apply(sdr, maps, bad)
    with pytest.raises(ValueError, match="map bytes"):
        K.gainmap_apply(sdr, maps[:-1], ap)
    torch.cuda.synchronize()


def test_stage_times_are_reported(shdr):
    K = shdr._ops
    sdr, hdr = R.content("noise", (65, 130), 5)
    images, _, _ = K.gainmap_images([(65, 130)], 2)
    ms = []
    K.gainmap_encode(dev(sdr).reshape(-1), dev(hdr).reshape(-1), images, stage_ms=ms)
    assert len(ms) == len(K.GAINMAP_STAGE_NAMES) == 3 and all(t >= 0 for t in ms)
