"""The parts of the deterministic mode that need no device (include/shdr.h "Deterministic mode"): the values of the workspace query -- the
pixel slices of the deterministic weight gradient depend on the layer alone -- and the refusals of the new entry points, all of which come
before the first launch.  Device pointers are stand-ins: a refused call never reads them."""
import ctypes

import pytest

E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5
(DET_WGRAD, DET_BIAS_GRAD, DET_ACT_BWD_BIAS, DET_BATCHNORM, DET_DIFF_LOSS, DET_TV_LOSS, DET_SAMPLE_DOT, DET_INVCRF, DET_APPLY_RF, DET_WINOGRAD,
 DET_X3) = range(11)
PTR = ctypes.c_void_p(1 << 20)                  # aligned, never dereferenced


@pytest.fixture(scope="module")
def K(shdr):
    return shdr._ops


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


def desc(K, x_shape, c2, k, cols, stride=1, algo=0):
    d = K._conv_desc(tuple(x_shape), (k, k, x_shape[3] + c2, cols), stride, c2, 1.0, cols)
    d.algo = algo
    return d


def test_constants_match_the_header(shdr):
    L = shdr._lib
    assert (L.DET_CONV2D_WGRAD, L.DET_BIAS_GRAD, L.DET_ACT_BWD_BIAS, L.DET_BATCHNORM, L.DET_DIFF_LOSS, L.DET_TV_LOSS, L.DET_SAMPLE_DOT,
            L.DET_INVCRF_DECODE_BWD, L.DET_APPLY_RF_BWD, L.DET_CONV2D_WGRAD_WINOGRAD, L.DET_CONV2D_WGRAD_X3) == tuple(range(11))


@pytest.mark.parametrize("case", [
    # x shape, c2, k, cols, stride, which, slices: why
    ((1, 47, 45, 32), 0, 3, 64, 1, 0, 3, "MFMA tiles: 2115 pixels in slices of 1024"),
    ((2, 47, 45, 96), 0, 7, 64, 2, 0, 2, "the stride-2 stem: 1104 output pixels"),
    ((1, 9, 16, 64), 0, 3, 64, 1, 0, 1, "144 pixels: one slice"),
    ((32, 64, 64, 256), 0, 3, 256, 1, 0, 14, "131072 pixels, 36 tiles of 64 x 128... : 512 / 36 = 14 slices"),
    ((1, 33, 50, 32), 32, 3, 32, 1, 1, 66, "all-taps: one slab per 32-pixel row segment up to 256"),
    ((1, 70, 150, 32), 0, 3, 16, 1, 0, 175, "all-taps: 350 segments, two per block"),
    ((1, 25, 41, 4), 0, 3, 16, 1, 0, 2, "direct kernel: slices of 1024 pixels"),
], ids=lambda c: c[7])
def test_weight_gradient_workspace(K, lib, case, monkeypatch):
    x_shape, c2, k, cols, stride, which, slices, _ = case
    monkeypatch.delenv("SHDR_NO_ALLTAPS", raising=False)          # a kernel-family switch: it picks the kernel, and with it the slices
    monkeypatch.setenv("SHDR_WGRAD_ROUNDS", "3")                   # ... while the grid experiments of the default form are ignored
    d = desc(K, x_shape, c2, k, cols, stride)
    slab = k * k * (x_shape[3] + c2) * cols * 4
    got = lib.shdr_det_workspace_bytes(DET_WGRAD, ctypes.byref(d), 0, which, 0)
    assert got == slices * slab, (got / slab, slices)


def test_winograd_and_split_operand_workspaces(K, lib):
    q = lib.shdr_det_workspace_bytes
    d = desc(K, (3, 33, 50, 32), 0, 3, 64)                           # 3 x 17 x 4 = 204 units of 2 x 16 pixels, 32 per slice: 7 slabs of dU
    assert q(DET_WINOGRAD, ctypes.byref(d), 0, 0, 0) == 7 * 16 * 32 * 64 * 4
    d = desc(K, (32, 64, 64, 256), 0, 3, 256)                        # 32 tiles: 512 / 32 = 16 slices of 4096 units
    assert q(DET_WINOGRAD, ctypes.byref(d), 0, 0, 0) == 16 * 16 * 256 * 256 * 4
    d = desc(K, (1, 33, 50, 64), 128, 3, 64)
    assert q(DET_WINOGRAD, ctypes.byref(d), 0, 1, 0) == 3 * 16 * 128 * 64 * 4 and q(DET_X3, ctypes.byref(d), 0, 1, 0) == 2 * 9 * 192 * 64 * 4
    d = desc(K, (32, 64, 64, 256), 0, 3, 256)                        # 9 taps x 2 x 2 tiles of 128: 512 / 36 = 14 slices
    assert q(DET_X3, ctypes.byref(d), 0, 0, 0) == 14 * 9 * 256 * 256 * 4
    d = desc(K, (1, 33, 50, 48), 0, 3, 64)                           # neither family takes 48 channels
    assert q(DET_WINOGRAD, ctypes.byref(d), 0, 0, 0) == -1 and q(DET_X3, ctypes.byref(d), 0, 0, 0) == -1
    assert q(DET_WINOGRAD, ctypes.byref(d), 0, 1, 0) == -1                                                   # no second source
    assert lib.shdr_conv2d_wgrad_winograd_det_f32(PTR, PTR, PTR, PTR, None, 1 << 30, 3, 33, 50, 32, 64, 32, 0, 1.0, None) == E_NULL
    assert lib.shdr_conv2d_wgrad_winograd_det_f32(PTR, PTR, PTR, PTR, PTR, 7 * 16 * 32 * 64 * 4 - 1, 3, 33, 50, 32, 64, 32, 0, 1.0, None) == E_SHAPE
    d = desc(K, (1, 33, 50, 64), 0, 3, 64)
    assert lib.shdr_conv2d_wgrad_x3_det_f32(ctypes.byref(d), PTR, PTR, 0, PTR, PTR, PTR, PTR, PTR, None, 1 << 30, None) == E_NULL
    assert lib.shdr_conv2d_wgrad_x3_det_f32(ctypes.byref(d), PTR, PTR, 0, PTR, PTR, PTR, PTR, PTR, PTR, 2 * 9 * 64 * 64 * 4 - 1, None) == E_SHAPE


def test_row_workspaces(lib):
    q = lib.shdr_det_workspace_bytes
    assert q(DET_BIAS_GRAD, None, 2115, 16, 0) == 3 * 16 * 4                     # 16 channels x 16 pixel lanes x 64 pixels per block
    assert q(DET_BIAS_GRAD, None, 10 ** 8, 16, 0) == 1024 * 16 * 4               # capped
    assert q(DET_ACT_BWD_BIAS, None, 2115, 64, 0) == 133 * 64 * 4
    assert q(DET_ACT_BWD_BIAS, None, 16384, 1024, 0) == 2048 * 1024 * 4 == lib.shdr_workspace_bytes(4, None, 1024)
    assert q(DET_ACT_BWD_BIAS, None, 2115, 6, 0) == -1                           # C % 4
    assert q(DET_BATCHNORM, None, 5000, 6, 0) == 2 * 6 * (1 + 3) * 8
    assert q(DET_BATCHNORM, None, 10 ** 8, 64, 0) == lib.shdr_workspace_bytes(3, None, 64)
    assert q(DET_DIFF_LOSS, None, 33000, 3, 0) == 128 * 3 * 4 and q(DET_SAMPLE_DOT, None, 257, 3, 0) == 2 * 3 * 4
    assert q(DET_TV_LOSS, None, 864, 0, 0) == 4 * 4 and q(DET_TV_LOSS, None, 10 ** 7, 0, 0) == 512 * 4
    assert q(DET_INVCRF, None, 0, 3, 255) == 3 * 256 * 11 * 4
    assert q(DET_APPLY_RF, None, 1027, 2, 1024) == 5 * 2 * 1024 * 4 and q(DET_APPLY_RF, None, 10 ** 7, 2, 1024) == 256 * 2 * 1024 * 4
    assert q(99, None, 1, 1, 1) == -1 and q(DET_BIAS_GRAD, None, 0, 16, 0) == -1 and q(DET_WGRAD, None, 0, 0, 0) == -1


def test_refusals_come_before_any_launch(K, lib):
    d = desc(K, (1, 47, 45, 32), 0, 3, 32)
    need = lib.shdr_det_workspace_bytes(DET_WGRAD, ctypes.byref(d), 0, 0, 0)
    f = lib.shdr_conv2d_wgrad_det_f32
    assert f(ctypes.byref(d), PTR, 0, PTR, PTR, None, need, None) == E_NULL
    assert f(ctypes.byref(d), PTR, 0, PTR, PTR, ctypes.c_void_p((1 << 20) + 4), need, None) == E_ALIGN
    assert f(ctypes.byref(d), PTR, 0, PTR, PTR, PTR, need - 1, None) == E_SHAPE and b"needed" in lib.shdr_last_error()
    assert f(ctypes.byref(d), None, 0, PTR, PTR, PTR, need, None) == E_NULL
    assert f(ctypes.byref(d), ctypes.c_void_p((1 << 20) + 4), 0, PTR, PTR, PTR, need, None) == E_ALIGN
    assert f(ctypes.byref(d), PTR, 1, PTR, PTR, PTR, need, None) == E_SHAPE                                   # no second source
    for algo in (4, 5, 6, 7):                                                                                   # fp16 / bf16 operands
        d.algo = algo
        assert f(ctypes.byref(d), PTR, 0, PTR, PTR, PTR, need, None) == E_SHAPE
        assert lib.shdr_det_workspace_bytes(DET_WGRAD, ctypes.byref(d), 0, 0, 0) == -1
    assert lib.shdr_bias_grad_det_f32(PTR, PTR, None, 1 << 20, 2115, 16, None) == E_NULL
    assert lib.shdr_bias_grad_det_f32(PTR, PTR, PTR, 3 * 16 * 4 - 1, 2115, 16, None) == E_SHAPE
    assert lib.shdr_act_bwd_bias_det_f32(PTR, None, None, PTR, None, 2115, 64, 0, None) == E_NULL
    assert lib.shdr_invcrf_decode_bwd_det_f32(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 3 * 256 * 11 * 4 - 1, 3, 255, 1024, None) == E_SHAPE
    assert lib.shdr_invcrf_decode_bwd_det_f32(PTR, PTR, PTR, PTR, PTR, PTR, PTR, None, 1 << 20, 3, 255, 1024, None) == E_NULL
    assert lib.shdr_apply_rf_bwd_det_f32(PTR, PTR, PTR, PTR, None, PTR, 1 << 30, 2, 1027, 8192, None) == E_SHAPE       # K <= 4096
    assert lib.shdr_apply_rf_bwd_det_f32(PTR, PTR, PTR, PTR, None, PTR, 5 * 2 * 1024 * 4 - 1, 2, 1027, 1024, None) == E_SHAPE
    assert lib.shdr_diff_loss_det_f32(PTR, PTR, PTR, None, 1 << 20, 3, 33000, 0, None) == E_NULL
    assert lib.shdr_diff_loss_det_f32(PTR, PTR, PTR, PTR, 128 * 3 * 4 - 1, 3, 33000, 0, None) == E_SHAPE
    assert lib.shdr_tv_loss_det_f32(PTR, PTR, PTR, 15, 2, 9, 16, 3, None) == E_SHAPE
    assert lib.shdr_sample_dot_det_f32(PTR, None, PTR, PTR, 2 * 3 * 4 - 1, 3, 257, None) == E_SHAPE
    assert lib.shdr_lin_frontend_bwd_det_f32(PTR, PTR, PTR, 1, 1, 5, 96, None) == E_SHAPE                     # H >= 2
    assert lib.shdr_lin_frontend_bwd_det_f32(PTR, None, PTR, 1, 2, 2, 96, None) == E_NULL


def test_switch_and_counter_without_a_device(K, shdr):
    assert K.DETERMINISTIC is False and K.order_dependent_launches() >= 0
    with K.deterministic(True):
        assert K.DETERMINISTIC is True
        with K.deterministic(False):
            assert K.DETERMINISTIC is False
        assert K.DETERMINISTIC is True
    assert K.DETERMINISTIC is False
    with pytest.raises(RuntimeError):
        with K.deterministic(True):
            raise RuntimeError("the scope ends with the exception")
    assert K.DETERMINISTIC is False
    before = K.order_dependent_launches()
    shdr._lib.load().shdr_bias_grad_f32(None, None, 10, 4, None)               # refused: a refused call is no launch
    assert K.order_dependent_launches() == before
