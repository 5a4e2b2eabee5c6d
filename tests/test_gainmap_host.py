"""CPU tests of the gain-map arithmetic: libshdr's host twins (K.gainmap_encode_host, K.gainmap_apply_host, csrc/gainmap.h) against
the float64 restatement of the rules (gainmap_ref.py).  No kernel is launched here.

THE TOLERANCES are derived from the measured errors of the header's polynomials (tools/gainmap_sweep.cpp; DESIGN.md "Gain maps"),
E = 5.649e-7 for log2_poly at the exponents -8 .. 8, E0 = 1.088e-7 at exponent 0 (where the result is the polynomial alone) and
X = 9.617e-8 (relative) for exp2_poly; u = 2^-24 is the unit round-off of fp32.

  codes   |code - 255 (g_ref - min_ref) / (max_ref - min_ref)| <= 0.5 + delta for EVERY cell and channel, with
          delta = 255 / (max_ref - min_ref) (2 E + E) + 255 * 4 u:
          2 E is twice the measured log2 error (g itself; its argument is computed in float64 and rounded to fp32 once, which moves g by
          at most u / (2 ln 2) = 4.3e-8, far inside the second E); the third E is the propagated error of min and max, each a g of some cell:
          |d code / d min| + |d code / d max| = 255 ((max - g) + (g - min)) / (max - min)^2 = 255 / (max - min); 4 u 255 is the fp32
          evaluation of the code formula itself (a difference, a product, a quotient, at most 255).  The reference is given the
          twin's s, so that this check is about the cells; s has its own check.
  min,max |min - min_ref| <= 2 E, |max - max_ref| <= 2 E + spacing(max) (the sum min + 2^-10 of the 2^-10 rule is rounded once).
  s       |log2 s - a_ref| <= 2 (E0 + spacing(lmax) / 2 + 3 u / ln 2) + spacing(a) / 2 + X / ln 2 + 2 u / ln 2: each of the two means is
          off by at most the error of one log2 (E0, plus the rounding of the exponent added to it, half a spacing at the largest
          |log2 Y| = lmax met) and the three roundings of a luminance (relative 3 u); a is rounded to fp32 once; exp2_poly adds X,
          and 2 u covers the rounding of log2 s in this test.
  apply   |out - out_ref| <= A_ref (X + ln 2 dL + 4 u) + u out_ref, A = (sdr + offset_sdr) 2^(L w) and dL the error of L w:
          dL = (|min| + |max|) 8 u + (max - min) dr + 2 spacing(|L w|), dr = 8 u for the bilinear mix (r <= 1, eight roundings),
          and with gamma != 1 dr = 8 u + X + ln 2 (E_r + spacing(log2 r / gamma)) with E_r = E0 + spacing(log2 r) / 2 <= E0 + 2^-21 for
          r >= 1 / 255 / 64.
"""
import numpy as np
import pytest

import gainmap_ref as R

LN2 = float(np.log(2.0))


def _arena(case):
    return case["sdr"].reshape(-1, 3), case["hdr"].reshape(-1, 3)


def _encode(K, case, log2_range=(-4.0, 8.0)):
    images, _, _ = K.gainmap_images([case["sdr"].shape[:2]], case["factor"])
    sdr, hdr = _arena(case)
    maps, meta = K.gainmap_encode_host(sdr, hdr, images, None if case["scale"] is None else [case["scale"]], log2_range, case["reverse"])
    H, W = case["sdr"].shape[:2]
    f = case["factor"]
    return maps.reshape(-(-H // f), -(-W // f), 3), meta[0]


def test_srgb_table_entry_by_entry(shdr):
    got = shdr._ops.gainmap_math_host("srgb")
    want = R.srgb_table()
    for i in range(256):
        assert got[i] == np.float32(want[i]), i


def test_polynomial_errors_stay_inside_the_measured_figures(shdr):
    """a sample of the sweep's measurement: the figures the tolerances are derived from hold on it"""
    K = shdr._ops
    rng = np.random.default_rng(7)
    m = np.concatenate([rng.integers(0, 1 << 23, 200000), [0, 1, (1 << 23) - 1, 0x3504F3, 0x3504F4]]).astype(np.uint32)
    for e in range(-8, 9):
        x = ((np.uint32(e + 127) << np.uint32(23)) | m).view(np.float32)
        err = np.abs(K.gainmap_math_host("log2", x).astype(np.float64) - np.log2(x.astype(np.float64))).max()
        assert err <= (R.E_LOG2_E0 if e == 0 else R.E_LOG2), (e, err)
    x = (rng.integers(-(16 << 16), (16 << 16) + 1, 400000) / 65536.0).astype(np.float32)
    rel = np.abs(K.gainmap_math_host("exp2", x).astype(np.float64) / np.exp2(x.astype(np.float64)) - 1).max()
    assert rel <= R.E_EXP2, rel
    assert K.gainmap_math_host("log2", [np.inf])[0] == 128.0 and K.gainmap_math_host("exp2", [np.nan])[0] == np.float32(2.0 ** -125)


@pytest.mark.parametrize("name", R.CONTENTS)
def test_codes_and_metadata_against_the_reference(shdr, name):
    K = shdr._ops
    worst = -1.0
    for case in R.cases(name):
        codes, meta = _encode(K, case)
        s = float(meta["scale"])
        # s
        if case["scale"] is not None:
            assert meta["scale"] == np.float32(case["scale"]) and meta["count"] == 0, case["name"]
        else:
            a, n = R.alignment(case["sdr"], case["hdr"], case["reverse"])
            assert meta["count"] == n, case["name"]
            if n == 0:
                assert s == 1.0, case["name"]
            else:
                h = R.sanitise(case["hdr"])[..., ::-1] if case["reverse"] else R.sanitise(case["hdr"])
                ok = ((case["sdr"] >= 16) & (case["sdr"] <= 239)).all(axis=-1)
                lmax = max(np.abs(np.log2(R.luminance(R.srgb_table()[case["sdr"]])[ok])).max(),
                           np.abs(np.log2(np.maximum(R.luminance(h)[ok], 2.0 ** -20))).max())
                bound = 2 * (R.E_LOG2_E0 + R.spacing32(lmax) / 2 + 3 * R.U / LN2) + R.spacing32(a) / 2 + R.E_EXP2 / LN2 + 2 * R.U / LN2
                assert abs(np.log2(s) - a) <= bound, (case["name"], np.log2(s) - a, bound)
        # cells
        g, mn, mx = R.gains(case["sdr"], case["hdr"], case["factor"], s, reverse=case["reverse"])
        assert abs(float(meta["gain_min"]) - mn) <= 2 * R.E_LOG2, (case["name"], float(meta["gain_min"]) - mn)
        assert abs(float(meta["gain_max"]) - mx) <= 2 * R.E_LOG2 + R.spacing32(mx), (case["name"], float(meta["gain_max"]) - mx)
        delta = 255.0 / (mx - mn) * 3 * R.E_LOG2 + 255 * 4 * R.U
        dev = np.abs(codes.astype(np.float64) - R.ideal_codes(g, mn, mx))
        assert dev.max() <= 0.5 + delta, (case["name"], dev.max(), delta)                       # every code: no exempt share
        worst = max(worst, dev.max() - 0.5)
    print("%s: largest |code - ideal| - 0.5 = %.3g" % (name, worst))


def test_case_list_meets_its_conditions():
    """conditions on the inputs, asserted on the reference: the constant image needs the 2^-10 rule, no_qualifying has no pixel for
    "auto", both_ends reaches both ends of the range, specials holds every special value"""
    for case in R.cases("constant"):
        g = R.gains(case["sdr"], case["hdr"], case["factor"], 1.0, reverse=case["reverse"])[0]
        assert g.max() - g.min() < 2.0 ** -10
    assert all(R.alignment(c["sdr"], c["hdr"], c["reverse"])[1] == 0 for c in R.cases("no_qualifying"))
    hit = [R.gains(c["sdr"], c["hdr"], c["factor"], 1.0, reverse=c["reverse"])[0] for c in R.cases("both_ends") if c["factor"] == 1]
    assert all(g.min() == -4.0 and g.max() == 8.0 for g in hit if g.size > 3)
    big = R.cases("specials")[-1]["hdr"]
    assert np.isnan(big).any() and np.isposinf(big).any() and np.isneginf(big).any() and (big < 0).any() and (big == 0).any() and (big > 1e29).any()
    assert any(c["reverse"] for c in R.cases("noise")) and any(not c["reverse"] for c in R.cases("noise"))
    assert any(c["scale"] is None for c in R.cases("noise")) and any(c["scale"] is not None for c in R.cases("noise"))


def test_a_narrow_range_clamps_both_ends(shdr):
    K = shdr._ops
    case = R.cases("noise")[-1]
    codes, meta = _encode(K, case, (-0.5, 0.25))
    assert meta["gain_min"] == -0.5 and meta["gain_max"] == 0.25
    g, mn, mx = R.gains(case["sdr"], case["hdr"], case["factor"], float(meta["scale"]), (-0.5, 0.25), case["reverse"])
    assert np.abs(codes - R.ideal_codes(g, mn, mx)).max() <= 0.5 + 255.0 / 0.75 * 3 * R.E_LOG2 + 255 * 4 * R.U
    assert (codes == 0).any() and (codes == 255).any()


def _apply_case(K, case, gamma, mc, weight, offsets=(1.0 / 64, 1.0 / 64)):
    codes, meta = _encode(K, case)
    if mc == 1:
        codes = np.ascontiguousarray(codes[:, :, 1:2])
    H, W = case["sdr"].shape[:2]
    images, _ = K.gainmap_apply_images([dict(height=H, width=W, factor=case["factor"], map_channels=mc, gain_min=meta["gain_min"],
                                             gain_max=meta["gain_max"], gamma=gamma, offset_sdr=offsets[0], offset_hdr=offsets[1], weight=weight)])
    got = K.gainmap_apply_host(case["sdr"].reshape(-1, 3), codes.reshape(-1), images).reshape(H, W, 3)
    im = images[0]
    mn, mx = float(im["gain_min"]), float(im["gain_max"])
    want, A = R.apply(case["sdr"], codes, case["factor"], mn, mx, float(im["gamma"]), float(im["offset_sdr"]), float(im["offset_hdr"]),
                      float(im["weight"]))
    dr = 8 * R.U
    if gamma != 1.0:
        dr += R.E_EXP2 + LN2 * (R.E_LOG2_E0 + 2.0 ** -21 + R.spacing32(14.0 / float(im["gamma"])))
    lw = max(abs(mn), abs(mx)) * float(im["weight"])
    dL = (abs(mn) + abs(mx)) * 8 * R.U + (mx - mn) * dr + 2 * R.spacing32(lw)
    bound = A * (R.E_EXP2 + LN2 * dL + 4 * R.U) + R.U * want
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (case["name"], gamma, mc, weight, float((err / bound).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("name", ["noise", "ramp", "specials"])
def test_apply_against_the_reference(shdr, name):
    K = shdr._ops
    worst = 0.0
    for i, case in enumerate(R.cases(name)):
        gamma, mc, weight = ((1.0, 3, 1.0), (2.2, 3, 0.6), (1.0, 1, 0.0), (0.8, 1, 1.0))[i % 4]
        worst = max(worst, _apply_case(K, case, gamma, mc, weight, (1.0 / 64, 1.0 / 64) if i % 3 else (0.03125, 0.0078125)))
    print("%s: largest error / bound = %.3g" % (name, worst))


def test_destinations_one_short_are_refused(shdr):
    K = shdr._ops
    case = R.cases("noise")[20]
    images, map_bytes, _ = K.gainmap_images([case["sdr"].shape[:2]], case["factor"])
    sdr, hdr = _arena(case)
    with pytest.raises(ValueError, match="the maps need"):
        K.gainmap_encode_host(sdr, hdr, images, map_capacity=map_bytes - 1)
    with pytest.raises(ValueError, match="meta records"):
        K.gainmap_encode_host(sdr, hdr, images, meta_capacity=0)
    codes, meta = _encode(K, case)
    H, W = case["sdr"].shape[:2]
    ap, _ = K.gainmap_apply_images([dict(height=H, width=W, factor=case["factor"], map_channels=3, gain_min=meta["gain_min"], gain_max=meta["gain_max"])])
    with pytest.raises(ValueError, match="destination"):
        K.gainmap_apply_host(sdr, codes.reshape(-1), ap, out_capacity=H * W - 1)
    with pytest.raises(ValueError, match="map bytes"):
        K.gainmap_apply_host(sdr, codes.reshape(-1)[:-1], ap)


def test_bad_descriptors_are_refused_by_name(shdr):
    K = shdr._ops
    with pytest.raises(ValueError, match="factor 3"):
        K.gainmap_images([(8, 8)], 3)
    with pytest.raises(ValueError, match="0 x 8"):
        K.gainmap_images([(0, 8)], 4)
    images, _, _ = K.gainmap_images([(8, 8)], 4)
    sdr, hdr = np.zeros((64, 3), np.uint8), np.zeros((64, 3), np.float32)
    outside = images.copy()
    outside["pix_off"] = 1
    with pytest.raises(ValueError, match="leaves the arenas"):
        K.gainmap_encode_host(sdr, hdr, outside)
    stale = images.copy()
    stale["cell_block0"] = 2
    with pytest.raises(ValueError, match="derived fields"):
        K.gainmap_encode_host(sdr, hdr, stale)
    with pytest.raises(ValueError, match="scale"):
        K.gainmap_encode_host(sdr, hdr, images, [0.0])
    with pytest.raises(ValueError, match="range"):
        K.gainmap_encode_host(sdr, hdr, images, log2_range=(2.0, 2.0))
