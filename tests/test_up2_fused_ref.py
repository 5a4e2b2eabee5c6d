"""The references of tests/test_gpu_up2_fused.py on their own (no device): every exact case meets its preconditions, the model of the
one-launch low-res form stays inside the bars of the GPU test at its shapes, and two deliberately wrong models of the fold leave them."""
import numpy as np
import pytest

import conv_ref as C
import up2_fused_ref as U


@pytest.mark.parametrize("o", U.EXACT_CASES, ids=[o["name"] for o in U.EXACT_CASES])
def test_every_exact_case_meets_its_preconditions(o):
    r = U.exact_reference(o)                                             # (asserts the three exactness preconditions)
    assert r["y"].shape == (o["n"], 2 * o["h"], 2 * o["w"], U.COUT) and r["yj"].shape == r["y"].shape[:3] + (3,)
    assert np.abs(r["yj"]).max() > 0 and (np.abs(r["proj"]).sum(axis=1) >= 2).all()


def test_the_exact_cases_cover_the_shapes_modes_and_epilogues():
    assert [(o["n"], o["h"], o["w"], o["cin"]) for o in U.EXACT_CASES] == U.SHAPES
    assert {o["mode"] for o in U.EXACT_CASES} == {"int", "fx", "fw", "fxw"}
    assert {o["epi"] for o in U.EXACT_CASES} == {"plain", "relu", "nobias", "up"}
    h = [s[1] for s in U.SHAPES]
    w = [s[2] for s in U.SHAPES]
    assert U.TILE_ROWS + 1 in h and U.TILE_COLS + 1 in w and max(h) > 2 * U.TILE_ROWS and max(w) > 2 * U.TILE_COLS


def test_fold_with_the_right_weights_is_the_stencil_of_conv_ref():
    rng = np.random.default_rng(5)
    z = rng.normal(size=(2, 5, 17, 9 * 4))
    assert np.array_equal(U.fold(z, 4), C.up2_lowres_stencil(z, 4)[0])


@pytest.mark.parametrize("shape, xscale", U.RANDOM_CASES, ids=["%s_x%g" % (U.shape_id(s), k) for s, k in U.RANDOM_CASES])
def test_model_stays_inside_the_bars_and_wrong_models_leave_them(shape, xscale):
    o = U.random_operands(shape, xscale)
    y, yj = U.oracle(o)
    my, mj = U.model(o)
    # the model differs from the ideal layer by the dropped xl wl products and the fp16 rounding of the weights' low terms only
    assert U.rel(my, y) <= U.TOL_PATHS and U.rel(mj, yj) <= U.TOL_PATHS, (U.rel(my, y), U.rel(mj, yj))
    n, h, w, _ = shape
    wrongs = [dict(near=0.25, far=0.75)] if h > 1 or w > 1 else []         # (a 1 x 1 image: both neighbours are the pixel itself)
    if w > U.TILE_COLS:
        wrongs.append(dict(tile_cols=U.TILE_COLS))
    for wrong in wrongs:
        wy, wj = U.model(o, **wrong)
        assert U.rel(wy, y) > 100 * U.TOL and U.rel(wj, yj) > 100 * U.TOL, (wrong, U.rel(wy, y), U.rel(wj, yj))
