"""Tensor-level wrappers around the libshdr C ABI.

PyTorch is used for device memory and streams only: every function here takes
NHWC float32 CUDA(HIP) tensors, allocates the output with torch and launches the
hand-written gfx950 kernel on torch's current stream through ctypes.  There is
no fallback path: CPU tensors or a missing library raise.
"""
import collections
import ctypes
import math

import numpy as np
import torch

try:
    from . import _lib
except ImportError:  # package directory itself on sys.path (drop-in module layout)
    import _lib

AUTOGRAD = None   # set by _autograd on import: module with the differentiable counterparts


def _needs_grad(*tensors):
    return AUTOGRAD is not None and torch.is_grad_enabled() and any(
        isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


WINOGRAD = True   # False: ask the library for the plain (non-Winograd) kernels only (experiments, tests)


ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
ALGO_AUTO, ALGO_MFMA, ALGO_DIRECT, ALGO_MFMA_REG = 0, 1, 2, 3
PROLOGUE_NONE, PROLOGUE_BILINEAR2X = 0, 1      # shdr_conv2d_desc.prologue
POOL_MAX, POOL_AVG = 0, 1                      # shdr_conv2d_desc.pool
ALGO_MFMA_F16, ALGO_MFMA_BF16, ALGO_AUTO_F16, ALGO_AUTO_BF16 = 4, 5, 6, 7
ALGO_AUTO_EXACT = 8    # AUTO without the split-operand fp16 kernel (plan "x3"): every product an fp32 FMA / fp32 MFMA
EXACT_FP32 = False     # True: ask the library for ALGO_AUTO_EXACT wherever this module would ask for ALGO_AUTO


def _auto(algo):
    return ALGO_AUTO_EXACT if (algo == ALGO_AUTO and EXACT_FP32) else algo

# Precision of the conv path.
#   "fp32"  : the parity path (exact-fp32 MFMA, Winograd where it pays).
#   "fp16"  : BASELINE configs[4], NATIVE fp16: the networks turn their inputs into fp16 feature maps (NHWC, C % 8 == 0) and every
#             conv forward / dgrad / wgrad, BatchNorm, pooling, resize and activation-backward pass reads and writes fp16
#             (csrc/conv_f16.hip, wgrad_f16.hip, elem_f16.hip); parameters, their gradients, statistics and the 3-channel
#             image-like tensors stay fp32, accumulation is fp32.  Ops dispatch on the dtype of their input tensor.
#   "fp16op" / "bf16" : the round-1 operand-rounding modes -- fp32 tensors in HBM, operands rounded when they are packed for
#             v_mfma_f32_16x16x32_{f16,bf16} (kept for comparison; Winograd is not used then).
PRECISION = "fp32"
_AUTO_ALGO = {"fp32": ALGO_AUTO, "fp16": ALGO_AUTO, "fp16op": ALGO_AUTO_F16, "bf16": ALGO_AUTO_BF16}


def native_fp16():
    """True inside `precision("fp16")`: feature maps are created as fp16"""
    return PRECISION == "fp16"


class precision:
    """with precision("fp16"): ...   -- scoped override of the conv operand precision"""

    def __init__(self, name):
        if name not in _AUTO_ALGO:
            raise ValueError("precision must be one of %s" % sorted(_AUTO_ALGO))
        self._name = name

    def __enter__(self):
        global PRECISION
        self._prev, PRECISION = PRECISION, self._name
        return self

    def __exit__(self, *exc):
        global PRECISION
        PRECISION = self._prev
        return False


# Deterministic mode (fp32 training path): inside `deterministic(True)` every reduction of a training step that ends in floating-point
# atomics by default -- weight / bias / BatchNorm / CRF-head gradients, the front end's backward, the loss sums -- runs its *_det_f32 form
# (include/shdr.h "Deterministic mode"): per-block slabs in a workspace of the call plus a fold in a fixed order.  Same inputs, same bits,
# run after run.  Not covered: the native-fp16 kernels (they raise here) and the collective across ranks.
DETERMINISTIC = False


class deterministic:
    """with deterministic(True): ...   -- scoped switch of the bit-reproducible forms of the fp32 training reductions"""

    def __init__(self, on=True):
        self._on = bool(on)

    def __enter__(self):
        global DETERMINISTIC
        self._prev, DETERMINISTIC = DETERMINISTIC, self._on
        return self

    def __exit__(self, *exc):
        global DETERMINISTIC
        DETERMINISTIC = self._prev
        return False


def order_dependent_launches():
    """launches so far, in this process, whose result depends on the arrival order of floating-point atomics (diagnostic, kept on the
    host by the library): it does not move over a step that ran on the deterministic forms alone"""
    return int(_lib.load().shdr_order_dependent_launches())


def _det_ws(op, device, d=None, n=0, c=0, k=0):
    """(workspace tensor of ONE deterministic call, its bytes): a fresh torch allocation per call, so two streams never share one"""
    nbytes = int(_lib.load().shdr_det_workspace_bytes(op, None if d is None else ctypes.byref(d), int(n), int(c), int(k)))
    if nbytes < 0:
        msg = _lib.load().shdr_last_error()
        raise ValueError("deterministic mode: no workspace size for op %d (n=%d, c=%d, k=%d): %s" % (op, n, c, k, msg.decode() if msg else ""))
    return torch.empty(max(nbytes, 16), device=device, dtype=torch.uint8), nbytes


def _no_det_h(what):
    if DETERMINISTIC:
        raise ValueError("%s: the deterministic mode does not cover the native-fp16 kernels yet" % what)


def same_pad(in_size, k, stride):
    """TF 'SAME': out = ceil(in/s); pad_before = max((out-1)*s + k - in, 0) // 2."""
    out = -(-in_size // stride)
    total = max((out - 1) * stride + k - in_size, 0)
    return out, total // 2


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s: tensor is on %s -- the SingleHDR hot path runs only on a HIP device "
                           "(no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (name, str(dtype).replace("torch.", ""), t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: tensor must be contiguous NHWC" % name)
    return t


HALF = torch.float16


def _is_h(t):
    return isinstance(t, torch.Tensor) and t.dtype == torch.float16


def _chkh(t, name):
    """fp16 feature map of the native-fp16 path: contiguous NHWC, C % 8 == 0"""
    t = _chk(t, name, torch.float16)
    if t.shape[-1] % 8:
        raise ValueError("%s: fp16 feature maps need C %% 8 == 0, got %d" % (name, t.shape[-1]))
    return t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _d(t):
    """detach parameters so that raw kernels can consume them"""
    return None if t is None else t.detach()


# ---------------------------------------------------------------------------
# tensors that one stream produces once and every stream consumes (per-version caches, constant slots)
# ---------------------------------------------------------------------------
class Ready:
    """Ordering of a cached tensor across streams.  The producer makes one right AFTER it has enqueued the work that writes the tensor(s):
    an event recorded on its stream.  Every consumer calls wait() before it enqueues a reader: on another stream than the producer's it
    waits for the event unless the event is already complete.  A complete event is dropped, so the steady state costs nothing: no launch,
    no device-side wait, and after the first answer not even a query.  No event calls while a stream capture is open (hipEventQuery invalidates the capture;
    GraphedInference warms the caches up first), and none for tensors that are not in device memory."""
    __slots__ = ("stream_id", "event")

    def __init__(self, device=None):
        self.stream_id = self.event = None
        if (device is None or device.type == "cuda") and not torch.cuda.is_current_stream_capturing():
            self.stream_id = torch.cuda.current_stream(device).cuda_stream
            self.event = torch.cuda.Event()
            self.event.record(torch.cuda.current_stream(device))

    def wait(self):
        event = self.event
        if event is None or torch.cuda.current_stream().cuda_stream == self.stream_id or torch.cuda.is_current_stream_capturing():
            return
        if event.query():
            self.event = None
        else:
            torch.cuda.current_stream().wait_event(event)


def _publish(t):
    """producer side for a single tensor: the Ready travels on the tensor"""
    t._shdr_ready = Ready(t.device)
    return t


def _consume(t):
    ready = getattr(t, "_shdr_ready", None)
    if ready is not None:
        ready.wait()
    return t


# ---------------------------------------------------------------------------
# range slots (include/shdr.h: shdr_conv2d_fwd_prepared_ranged_f32)
# ---------------------------------------------------------------------------
# The split-operand conv plans scale their input by a power of two taken from a RANGE SLOT: a device float holding an upper bound of
# max |x| of the tensor.  The kernels that produce a tensor write its slot from their epilogue (`y_range`), bound-preserving ops
# (pooling, bilinear resize, clip, channel reversal) hand their input's slot on, host-known bounds become constant slots, and a tensor
# that arrives without one is measured by the library (one pass over it).  A tensor's range travels as ONE record: the attributes
# `_shdr_range` (slot), `_shdr_bound` (host bound) and `_shdr_range_ver` (the t._version both describe), written together by _set_range.
#   R1  a read checks the version for both kinds: an in-place update (autograd accumulating a second gradient into a buffer) voids them.
#   R2  a bound that is not finite is not recorded (the kernels read one as "scale 1, measure nothing").
#   R3  raw-pointer writes bump no version: _conv2d_raw drops `out`'s record before any launch, then attaches the slot a kernel wrote.
#   R4  fp32 add(a, b, relu=True) hands the sum's measured slot on (|relu(s)| <= |s|) instead of clip's infinite bound.
_RANGE_SCOPES = []
_CONST_SLOTS = {}


class range_scope:
    """Slots taken inside the scope come out of ONE zero-initialised slab (one memset per step instead of one per tensor).  The step
    closures of `pipeline` open a scope per forward and per stream; outside a scope every slot is its own zeroed one-element tensor."""

    SLOTS = 256

    def __enter__(self):
        self._slabs = {}                   # (device, stream) -> [slab, slots taken]
        _RANGE_SCOPES.append(self)
        return self

    def __exit__(self, *exc):
        _RANGE_SCOPES.remove(self)
        return False

    def take(self, device):
        # one slab per stream: its zero-fill is ordered in front of the kernels that write its slots by the stream itself (the backward
        # pass of a multi-stream step takes slots on the stream of each node's forward op)
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        ent = self._slabs.get(key)
        if ent is None or ent[1] == self.SLOTS:
            ent = self._slabs[key] = [torch.zeros(self.SLOTS, device=device, dtype=torch.float32), 0]
        ent[1] += 1
        return ent[0][ent[1] - 1:ent[1]]


PROJECTED_LAUNCHES = [0]                  # convolutions that wrote a projected output from their epilogue (diagnostic / tests)
RANGE_MISSES = collections.Counter()      # split-operand layers whose input arrived without a range (diagnostic: each costs one pass over x)


def _new_slot(device):
    if _RANGE_SCOPES:
        return _RANGE_SCOPES[-1].take(device)
    return torch.zeros(1, device=device, dtype=torch.float32)


def _record(t):
    """(slot, bound) of t's range record if it still describes t (R1), else (None, None) -- also for t None"""
    ver = getattr(t, "_shdr_range_ver", None)
    return (t._shdr_range, t._shdr_bound) if ver is not None and ver == t._version else (None, None)


def _range_of(t):
    """the range slot of a tensor (1-element fp32 device tensor) or None; a host-known bound becomes a constant slot"""
    slot, b = _record(t)
    if slot is not None or b is None:
        return slot
    slot = _CONST_SLOTS.get((t.device, b))
    if slot is None:
        slot = _CONST_SLOTS[(t.device, b)] = _publish(torch.full((1,), b, device=t.device, dtype=torch.float32))
    return _consume(slot)        # (filled on whichever stream asked first)


def _bound_of(t):
    """the host-known upper bound of max |t| or None"""
    return _record(t)[1]


def _set_range(t, slot, bound=None):
    t._shdr_range, t._shdr_bound, t._shdr_range_ver = slot, bound, t._version
    return t


def _carry_range(y, x):
    """y is bounded by x's bound (pooling, convex resampling, channel permutation, clipping of an already bounded tensor, the
    derivative of an activation applied to a gradient)"""
    return _set_range(y, *_record(x))


def set_bound(t, bound):
    """declare a host-known upper bound of max |t| (e.g. an image in [0, 1]); a non-finite one declares nothing (R2)"""
    b = float(bound)
    return _set_range(t, None, b if math.isfinite(b) else None)


def absmax_slot(x):
    """measure max |x| into a fresh range slot and attach it to x"""
    lib = _lib.load()
    xd = _chk(_d(x), "x")
    slot = _new_slot(xd.device)
    _lib.check(lib.shdr_absmax_f32(_ptr(xd), xd.numel(), _ptr(slot), _stream()), "shdr_absmax_f32")
    _set_range(x, slot)
    return slot


def conv2d(x, w, bias=None, stride=1, x2=None, x2_scale=1.0, act1=ACT_NONE, scale=None,
           shift=None, residual=None, act2=ACT_NONE, algo=ALGO_AUTO, out=None, cout_valid=None,
           pad=None, out_hw=None, w_batch_stride=0):
    """y = act2(affine(act1(conv(concat[x, x2_scale*x2], w) + bias)) + residual), SAME padding.

    `cout_valid` < w.shape[3] says the filter is zero-padded along Cout (to a multiple of 16 so
    that a narrow head runs on the MFMA tile); only the first `cout_valid` channels are stored.
    `pad=(top, left)` / `out_hw=(Ho, Wo)` override the SAME rule (used by the strided dgrad)."""
    if _is_h(x):
        fused = scale is not None or shift is not None or residual is not None or act2 != ACT_NONE
        if pad is not None or out is not None or w_batch_stride or algo != ALGO_AUTO:
            raise NotImplementedError("conv2d: the native-fp16 path takes no pad / out / w_batch_stride / algo")
        if _needs_grad(x, x2, w, bias, scale, shift, residual):
            if fused:
                raise NotImplementedError("conv2d: the native-fp16 path takes bias + act1 only on a gradient tape (training-mode layers)")
            return AUTOGRAD.conv2d_h(x, w, bias, stride, x2, x2_scale, act1, cout_valid)
        # tape-free: the inference epilogue (folded BatchNorm, residual, act2) fused into the fp16 kernels (shdr_conv2d_fwd_fused_f16)
        return conv2d_h(x, pack_filter_h(w, x.shape[3], 0 if x2 is None else x2.shape[3], x2_scale), bias, tuple(w.shape[:2]),
                        w.shape[3], stride=stride, x2=x2, act1=act1, cout_valid=cout_valid, scale=scale, shift=shift,
                        residual=residual, act2=act2)
    if algo == ALGO_AUTO:
        algo = _AUTO_ALGO[PRECISION]
    fused = scale is not None or shift is not None or residual is not None or act2 != ACT_NONE
    if _needs_grad(x, x2, w, bias, scale, shift, residual):
        if pad is not None or out_hw is not None or out is not None or w_batch_stride:
            raise NotImplementedError("conv2d: pad / out_hw / out / w_batch_stride are raw-kernel options (input-gradient and "
                                      "Winograd plumbing) and cannot be recorded on a gradient tape")
        y = AUTOGRAD.conv2d(x, w, bias, stride=stride, x2=x2, x2_scale=x2_scale, act1=act1, algo=algo, cout_valid=cout_valid)
        if not fused:
            return y
        # A fused inference epilogue (folded BatchNorm, residual join, second activation) under a tape -- e.g.
        # `lin(x, training=False)` while fine-tuning with frozen BatchNorm statistics: recorded as conv + affine/join/activation,
        # two tape entries, instead of silently returning a tensor that is cut off from the graph.
        return AUTOGRAD.affine_act(y, scale, shift, residual, act2)
    return _conv2d_raw(x, w, bias, stride, x2, x2_scale, act1, scale, shift, residual, act2, algo, out, cout_valid, pad, out_hw,
                       w_batch_stride, None)


def conv2d_up2(x, w, bias=None, act1=ACT_NONE, scale=None, shift=None, act2=ACT_NONE, proj=None, lowres=False, one_launch=False):
    """Conv2D(SAME, stride 1)(tf.image.resize(x, 2x, BILINEAR)) with the conv2d epilogue -- the `up` blocks of
    hallucination_net.py:86-88 and dequantization_net.py:25-27.  Without a gradient tape the library fuses the resize into the
    convolution where the plan allows it (desc.prologue, csrc/conv_plan.hip); under a tape, and in the reduced-precision operand
    modes, it is the two recorded ops.
    proj [3, Cout]: the PROJECTED output sum_c proj[j, c] y[..., c] instead of y (include/shdr.h:
    shdr_conv2d_fwd_prepared_projected_f32), or None when the planned kernel of the layer cannot form it.
    lowres=True: the caller accepts the form that mixes the channels at LOW resolution (csrc/up2_lowres.hip: a 1x1 GEMM Cin -> 9 Cout on
    x, then a stencil pass; the accuracy class of the split-operand kernels, not the bits of the default form) where the library takes the
    layer (shdr_conv2d_up2_lowres_ok_f32); elsewhere, and with the default, this is the call below.  With proj it is the one-launch
    form of the same arithmetic (csrc/up2_fused.hip, shdr_conv2d_up2_fused_ok_f32), which writes the projected output alone.
    one_launch=True (with lowres=True, without proj): the one-launch form comes first where its predicate takes the layer (16, 32 or 64
    couts, at most 128 input channels: the `up` blocks of the Dequantization-Net), then the two-launch form; not under
    SHDR_NO_UP2_NARROW=1."""
    if lowres and proj is not None and not _is_h(x) and _AUTO_ALGO[PRECISION] == ALGO_AUTO and WINOGRAD and not EXACT_FP32 \
            and not _needs_grad(x, w, bias, scale, shift):
        yj = _conv2d_up2_fused(x, w, bias, act1, scale, shift, act2, proj)
        if yj is not None:
            return yj
    if lowres and proj is None and not _is_h(x) and _AUTO_ALGO[PRECISION] == ALGO_AUTO and WINOGRAD and not EXACT_FP32 \
            and not _needs_grad(x, w, bias, scale, shift):
        if one_launch and up2_narrow_enabled():
            y = _conv2d_up2_fused(x, w, bias, act1, scale, shift, act2)
            if y is not None:
                return y
        y = _conv2d_up2_lowres(x, w, bias, act1, scale, shift, act2)
        if y is not None:
            return y
    algo = _AUTO_ALGO[PRECISION]
    if _is_h(x) or algo != ALGO_AUTO or not WINOGRAD or _needs_grad(x, w, bias, scale, shift):
        if proj is not None:
            return None
        return conv2d(resize2x(x), w, bias, act1=act1, scale=scale, shift=shift, act2=act2)
    return _conv2d_raw(x, w, bias, 1, None, 1.0, act1, scale, shift, None, act2, algo, None, None, None, None, 0, None,
                       prologue=PROLOGUE_BILINEAR2X, proj=proj)


def up2_narrow_enabled():
    """False under SHDR_NO_UP2_NARROW=1: the A/B arm in which the `up` blocks of the Dequantization-Net stay on the bilinear-prologue
    kernels (the library reads the switch: shdr_conv2d_up2_narrow_enabled)"""
    return bool(_lib.load().shdr_conv2d_up2_narrow_enabled())


def _up2_layer(form, x, w, bias, act1, scale, shift, act2):
    """(descriptor, x, prepared filter) of conv2d_up2 on one of the low-res forms -- "lowres": csrc/up2_lowres.hip, "fused":
    csrc/up2_fused.hip -- or None where the library does not take the layer.  The descriptor is that of _conv2d_raw's bilinear-prologue
    call; the prepared filter is kept on the variable per version under a key of the form's own."""
    lib = _lib.load()
    x, w_var = _d(x), w
    w = _d(w)
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[:2]) != (3, 3) or w.shape[2] != x.shape[3]:
        return None
    n, h, wd, c1 = x.shape
    cout = w.shape[3]
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C1, d.C2 = n, 2 * h, 2 * wd, c1, 0
    d.Cout, d.KH, d.KW, d.stride = cout, 3, 3, 1
    d.cout_valid, d.y_cstride = cout, cout
    d.pad_t, d.pad_l, d.Ho, d.Wo = 1, 1, 2 * h, 2 * wd
    d.x2_scale = 1.0
    d.act1, d.act2 = act1, act2
    d.algo = ALGO_AUTO
    d.prologue = PROLOGUE_BILINEAR2X
    if not int(getattr(lib, "shdr_conv2d_up2_%s_ok_f32" % form)(ctypes.byref(d))):
        return None
    _chk(x, "x")
    _chk(w, "w")
    for t, nm in ((bias, "bias"), (scale, "scale"), (shift, "shift")):
        if t is not None and (_chk(_d(t), nm).numel() != cout):
            raise ValueError("conv2d_up2: %s must have %d elements" % (nm, cout))
    persistent = _is_persistent(w_var)
    nprep = int(getattr(lib, "shdr_conv2d_up2_%s_filter_elems_f32" % form)(ctypes.byref(d)))      # (follows the padding of the GEMM's columns)
    key = ("up2_" + form, c1, cout, nprep)
    prepared = _filter_cache_get(w_var, "_shdr_packed", key) if persistent else None
    if prepared is None:
        prepared = torch.empty(nprep, device=w.device, dtype=torch.float32)
        name = "shdr_conv2d_up2_%s_prepare_filter_f32" % form
        _lib.check(getattr(lib, name)(ctypes.byref(d), _ptr(w), _ptr(prepared), _stream()), name)
        if persistent:
            _filter_cache_put(w_var, "_shdr_packed", key, prepared)
    return d, x, prepared


def _conv2d_up2_lowres(x, w, bias, act1, scale, shift, act2):
    """conv2d_up2 through shdr_conv2d_fwd_up2_lowres_f32, or None where the library does not take the layer.  Plumbing only."""
    layer = _up2_layer("lowres", x, w, bias, act1, scale, shift, act2)
    if layer is None:
        return None
    lib = _lib.load()
    x_in = x
    d, x, prepared = layer
    xr = _range_of(x_in)
    if xr is None:
        RANGE_MISSES[(tuple(x.shape), None, tuple(_d(w).shape))] += 1     # measured below the ABI
    ws = torch.empty(int(lib.shdr_conv2d_up2_lowres_workspace_bytes_f32(ctypes.byref(d))), device=x.device, dtype=torch.uint8)
    out = torch.empty((d.N, d.H, d.W, d.Cout), device=x.device, dtype=torch.float32)
    yr = _new_slot(x.device)
    rc = lib.shdr_conv2d_fwd_up2_lowres_f32(ctypes.byref(d), _ptr(x), _ptr(prepared), _ptr(_d(bias)), _ptr(_d(scale)), _ptr(_d(shift)),
                                            _ptr(out), _ptr(ws), _ptr(xr), _ptr(yr), _stream())
    _lib.check(rc, "shdr_conv2d_fwd_up2_lowres_f32")
    return _set_range(out, yr)


def _conv2d_up2_fused(x, w, bias, act1, scale, shift, act2, proj=None, want_y=None):
    """conv2d_up2 through shdr_conv2d_fwd_up2_fused_f32, or None where the library does not take the layer: the projected output
    [N, 2h, 2w, 3] for proj [3, 64], y (the bits of _conv2d_up2_lowres) without one, (y_proj, y) with want_y=True.  Plumbing only."""
    if proj is not None and _d(w).shape[-1] != 64:                    # the projected output is the 64-cout form's
        return None
    layer = _up2_layer("fused", x, w, bias, act1, scale, shift, act2)
    if layer is None:
        return None
    lib = _lib.load()
    x_in = x
    d, x, prepared = layer
    if proj is not None:
        proj = _chk(_d(proj), "proj")
        if tuple(proj.shape) != (3, d.Cout):
            raise ValueError("conv2d_up2: proj must be [3, %d]" % d.Cout)
    if want_y is None:
        want_y = proj is None
    xr = _range_of(x_in)
    if xr is None:                                                    # measured here: the entry takes the slot, not a workspace
        RANGE_MISSES[(tuple(x.shape), None, tuple(_d(w).shape))] += 1
        xr = _new_slot(x.device)
        _lib.check(lib.shdr_absmax_f32(_ptr(x), x.numel(), _ptr(xr), _stream()), "shdr_absmax_f32")
    out = torch.empty((d.N, d.H, d.W, d.Cout), device=x.device, dtype=torch.float32) if want_y else None
    yj = torch.empty((d.N, d.H, d.W, 3), device=x.device, dtype=torch.float32) if proj is not None else None
    yr = _new_slot(x.device) if want_y else None
    rc = lib.shdr_conv2d_fwd_up2_fused_f32(ctypes.byref(d), _ptr(x), _ptr(prepared), _ptr(_d(bias)), _ptr(_d(scale)), _ptr(_d(shift)),
                                           _ptr(proj), _ptr(yj), _ptr(out), _ptr(xr), _ptr(yr), _stream())
    _lib.check(rc, "shdr_conv2d_fwd_up2_fused_f32")
    if proj is not None:
        PROJECTED_LAUNCHES[0] += 1
    if want_y:
        _set_range(out, yr)
    return out if proj is None else ((yj, out) if want_y else yj)


def _conv2d_raw(x, w, bias, stride, x2, x2_scale, act1, scale, shift, residual, act2, algo, out, cout_valid, pad, out_hw,
                w_batch_stride, pool, prologue=0, proj=None):
    """One convolution through the C ABI.  The kernel family (one-kernel Winograd, three-kernel Winograd, register-A / LDS-DMA
    implicit GEMM, direct) is chosen BELOW the ABI (shdr_conv2d_plan_f32, csrc/conv_plan.hip); this wrapper only checks shapes,
    caches the prepared filter of persistent variables per version and provides memory.  pool: None, True (also return
    MaxPool2D(2)(y)), "only" (the pooled tensor alone) or "avg" (also return AveragePooling2D(2)(y)).
    proj [3, Cout]: return the PROJECTED output [N, Ho, Wo, 3] (sum_c proj[j, c] y[..., c]) instead of y -- (y_proj, pooled) with a
    pool -- or None when the layer's planned kernel cannot form it (conv2d_projected falls back to two convolutions)."""
    lib = _lib.load()
    x_in, x2_in = x, x2                # the tensors as handed over: they carry the range slots (a detached copy does not)
    x = _chk(_d(x), "x")
    w_var = w                          # the variable itself: its version / leaf status key the prepared-filter cache
    w = _chk(_d(w), "w")
    n, h, wd, c1 = x.shape
    if prologue == PROLOGUE_BILINEAR2X:
        h, wd = 2 * h, 2 * wd              # the descriptor describes the convolution: its input is the up-sampled image
    kh, kw, cin, cout_gemm = w.shape
    cout = cout_gemm if cout_valid is None else int(cout_valid)
    c2 = 0
    if x2 is not None:
        x2 = _chk(_d(x2), "x2")
        if x2.shape[:3] != x.shape[:3]:
            raise ValueError("conv2d: x2 spatial shape %s != x %s" % (tuple(x2.shape), tuple(x.shape)))
        c2 = x2.shape[3]
    if cin != c1 + c2:
        raise ValueError("conv2d: filter expects %d input channels, got %d+%d" % (cin, c1, c2))
    ho, pt = same_pad(h, kh, stride)
    wo, pl = same_pad(wd, kw, stride)
    if pad is not None:
        pt, pl = pad
    if out_hw is not None:
        ho, wo = out_hw
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C1, d.C2 = n, h, wd, c1, c2
    d.Cout, d.KH, d.KW, d.stride = cout_gemm, kh, kw, stride
    d.cout_valid = cout
    d.pad_t, d.pad_l, d.Ho, d.Wo = pt, pl, ho, wo
    d.x2_scale = float(x2_scale)
    d.act1, d.act2 = act1, act2
    d.algo = _auto(algo)
    d.w_batch_stride = int(w_batch_stride)
    d.prologue = int(prologue)
    d.pool = POOL_AVG if pool == "avg" else POOL_MAX
    res_cs = 0
    if residual is not None:
        residual = _chk(_d(residual), "residual")
        if tuple(residual.shape[:3]) != (n, ho, wo) or residual.shape[3] < cout:
            raise ValueError("conv2d: residual shape %s incompatible with output [%d,%d,%d,%d]"
                             % (tuple(residual.shape), n, ho, wo, cout))
        res_cs = residual.shape[3]
    d.res_cstride = res_cs
    if proj is not None:
        if algo != ALGO_AUTO or not WINOGRAD or residual is not None or not int(lib.shdr_conv2d_projected_ok_f32(ctypes.byref(d))):
            return None
        proj = _chk(_d(proj), "proj")
        if tuple(proj.shape) != (3, cout):
            raise ValueError("conv2d: proj must be [3, %d]" % cout)
    elif out is None:
        out = None if pool == "only" else torch.empty((n, ho, wo, cout), device=x.device, dtype=torch.float32)
    else:
        _chk(out, "out")
        if tuple(out.shape) != (n, ho, wo, cout):
            raise ValueError("conv2d: bad out shape")
        _set_range(out, None)          # R3: the kernels below write out through a raw pointer
    d.y_cstride = cout
    for t, nm, ln in ((bias, "bias", cout), (scale, "scale", cout), (shift, "shift", cout)):
        if t is not None and (_chk(_d(t), nm).numel() != ln):
            raise ValueError("conv2d: %s must have %d elements" % (nm, ln))
    if algo != ALGO_AUTO or not WINOGRAD:
        # explicit kernel family / reduced-precision operand modes / Winograd switched off: the plain entry point
        if pool:
            raise ValueError("conv2d: the pooled output needs algo AUTO")
        rc = lib.shdr_conv2d_fwd_f32(ctypes.byref(d), _ptr(x), _ptr(x2), _ptr(w), _ptr(_d(bias)),
                                     _ptr(_d(scale)), _ptr(_d(shift)), _ptr(residual), _ptr(out), _stream())
        _lib.check(rc, "shdr_conv2d_fwd_f32")
        return out
    has_res = int(residual is not None)
    prepared = _prepared_filter(lib, w_var, d, has_res)
    plan = int(lib.shdr_conv2d_plan_f32(ctypes.byref(d), has_res))
    split = plan in (4, 5)             # SHDR_PLAN_X3 / X3N: the input is scaled by its range, the epilogue tracks the output's
    xr1 = _range_of(x_in) if split else None
    xr2 = _range_of(x2_in) if (split and x2 is not None) else None
    if split and (xr1 is None or (x2 is not None and xr2 is None)):
        RANGE_MISSES[(tuple(x.shape), None if x2 is None else tuple(x2.shape), tuple(w.shape))] += 1     # measured below the ABI
    ws = None
    nws = int(lib.shdr_conv2d_workspace_bytes_f32(ctypes.byref(d), has_res))
    if nws > 256 or (nws > 0 and (not split or xr1 is None or (x2 is not None and xr2 is None))):
        ws = torch.empty(nws, device=x.device, dtype=torch.uint8)      # (a split plan with known ranges needs no scratch slots)
    yp = None
    if pool:
        if ho % 2 or wo % 2:
            raise ValueError("conv2d: pool needs even output height / width")
        yp = torch.empty((n, ho // 2, wo // 2, cout), device=x.device, dtype=torch.float32)
        if out is None and plan not in (2, 4):      # the fused Winograd and split kernels can skip y
            out = torch.empty((n, ho, wo, cout), device=x.device, dtype=torch.float32)
    # the output's range slot: written by the epilogue of the split-operand and of the exact-fp32 MFMA / direct kernels (no extra pass)
    yr = _new_slot(x.device) if (split or (plan in (0, 1) and prologue == PROLOGUE_NONE and out is not None)) else None
    if proj is not None:
        yj = torch.empty((n, ho, wo, 3), device=x.device, dtype=torch.float32)
        rc = lib.shdr_conv2d_fwd_prepared_projected_f32(ctypes.byref(d), _ptr(x), _ptr(x2), _ptr(prepared), _ptr(_d(bias)), _ptr(_d(scale)),
                                                        _ptr(_d(shift)), _ptr(proj), _ptr(yj), None, _ptr(yp), _ptr(ws), _ptr(xr1),
                                                        _ptr(xr2), _ptr(yr), _stream())
        _lib.check(rc, "shdr_conv2d_fwd_prepared_projected_f32")
        PROJECTED_LAUNCHES[0] += 1
        if yp is not None:
            _set_range(yp, yr)             # (the pooled copy of y is bounded by max |y|)
        return (yj, yp) if pool else yj
    rc = lib.shdr_conv2d_fwd_prepared_ranged_f32(ctypes.byref(d), _ptr(x), _ptr(x2), _ptr(prepared), _ptr(_d(bias)), _ptr(_d(scale)),
                                                 _ptr(_d(shift)), _ptr(residual), _ptr(out), _ptr(yp), _ptr(ws), _ptr(xr1), _ptr(xr2),
                                                 _ptr(yr), _stream())
    _lib.check(rc, "shdr_conv2d_fwd_prepared_ranged_f32")
    if yr is not None:
        for t in (out, yp):
            if t is not None:
                _set_range(t, yr)          # (the pooled copy is bounded by the same maximum)
    if pool == "only":
        return yp
    return (out, yp) if pool else out


def _is_persistent(w):
    """requires_grad leaves (the layers' kernels) and frozen constants (_shdr_const: VGG16, padded / composed filters)"""
    return (w.requires_grad and w.is_leaf) or getattr(w, "_shdr_const", False)


def _filter_cache_get(w, attr, key):
    """Derived forms of a persistent filter (prepared / packed / fp16-packed) live ON the filter tensor in a dict
    {key: (tensor, Ready)} tagged with the variable's version.  Entries are dropped only when the version
    changes: the same weight takes different plans at different input shapes (x3 needs >= 192 blocks, x3n >= 256 tiles), and a
    captured HIP graph holds the raw pointer of the form it was captured with -- evicting one shape's form for another's would
    leave that graph reading freed memory.  A consumer on another stream than the producer waits for the producer's event (Ready)."""
    store = getattr(w, attr, None)
    if store is None or store[0] != w._version:
        return None
    ent = store[1].get(key)
    if ent is None:
        return None
    ent[1].wait()
    return ent[0]


def _filter_cache_put(w, attr, key, tensor):
    store = getattr(w, attr, None)
    if store is None or store[0] != w._version:
        store = (w._version, {})
        setattr(w, attr, store)
    store[1][key] = (tensor, Ready(tensor.device))
    return tensor


def clear_filter_caches(w):
    """forget every derived form kept on a filter tensor (the tensor moved to another device, or was rewritten behind torch's back)"""
    for attr in ("_shdr_packed", "_shdr_packed_h", "_shdr_wino"):
        if hasattr(w, attr):
            delattr(w, attr)


def _prepared_filter(lib, w, d, has_res):
    """shdr_conv2d_prepare_filter_f32(w) for the plan of this layer -- `w` itself when the library says the prepared form is the
    plain filter; kept ON the filter tensor per version and per (plan, sources, skip scale) for persistent variables
    (requires_grad leaves: the layers' kernels, frozen VGG16 constants), so an inference step prepares nothing; temporaries
    (transposed dgrad filters) per call.  Every kernel that rewrites a variable through a raw pointer bumps its version
    (_mutated, KerasAdam)."""
    if int(lib.shdr_conv2d_filter_is_plain_f32(ctypes.byref(d), has_res)):
        return _d(w)
    persistent = _is_persistent(w)
    key = None
    if persistent:
        key = (int(lib.shdr_conv2d_plan_f32(ctypes.byref(d), has_res)), d.C1, d.C2, float(d.x2_scale))
        cached = _filter_cache_get(w, "_shdr_packed", key)
        if cached is not None:
            return cached
    n = int(lib.shdr_conv2d_prepared_filter_elems_f32(ctypes.byref(d), has_res))
    prepared = torch.empty(n, device=w.device, dtype=torch.float32)
    _lib.check(lib.shdr_conv2d_prepare_filter_f32(ctypes.byref(d), has_res, _ptr(_d(w)), _ptr(prepared), _stream()),
               "shdr_conv2d_prepare_filter_f32")
    if persistent:
        _filter_cache_put(w, "_shdr_packed", key, prepared)
    return prepared


_PLAN_NAMES = {0: "direct", 1: "mfma", 2: "fused", 3: "planes", 4: "x3", 5: "x3n"}


def conv2d_plan(x_shape, w_shape, c2=0, stride=1, x2_scale=1.0, has_residual=False, cout_valid=None):
    """the kernel family shdr_conv2d_fwd_prepared_f32 runs for a SAME-padded layer: "fused" (one-kernel Winograd), "planes"
    (three-kernel Winograd), "mfma" (register-A / LDS-DMA implicit GEMM) or "direct" -- asked from the library, not decided here"""
    lib = _lib.load()
    n, h, wd, c1 = x_shape
    kh, kw, cin, cout = w_shape
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C1, d.C2 = n, h, wd, c1, c2
    d.Cout, d.KH, d.KW, d.stride = cout, kh, kw, stride
    d.cout_valid = cout_valid or cout
    d.Ho, d.pad_t = same_pad(h, kh, stride)
    d.Wo, d.pad_l = same_pad(wd, kw, stride)
    d.x2_scale = float(x2_scale)
    d.algo = _auto(ALGO_AUTO) if WINOGRAD else ALGO_MFMA
    return _PLAN_NAMES[int(lib.shdr_conv2d_plan_f32(ctypes.byref(d), int(has_residual)))]


def winograd_path(cin, cout):
    """"fused" / "planes" / None for a single-source 3x3 stride-1 layer with these channel counts (library policy)"""
    p = conv2d_plan((1, 64, 64, cin), (3, 3, cin, cout))
    return p if p in ("fused", "planes") else None


def conv2d_dgrad(dz, w, x_shape, c1, c2, which, stride=1, x2_scale=1.0):
    """dx [x_shape] of the SAME-padded forward conv(concat[x1 (c1 ch), x2_scale * x2 (c2 ch)], w) w.r.t. source `which` from
    dz = dL/d(conv output) [N,Ho,Wo,cout_valid]: ONE library call (shdr_conv2d_dgrad_f32: filter flip / slice / zero-padding,
    Winograd where the transposed layer qualifies, 1x1 / 2 on the coarse grid, polyphase form for general stride 2)."""
    lib = _lib.load()
    dz_in = dz
    dz, w = _chk(_d(dz), "dz"), _chk(_d(w), "w")
    n, h, wd, cx = x_shape
    kh, kw, cin, cout = w.shape
    if cin != c1 + c2 or cx != (c2 if which else c1):
        raise ValueError("conv2d_dgrad: filter %s / sources %d+%d / x %s do not match" % (tuple(w.shape), c1, c2, tuple(x_shape)))
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C1, d.C2 = n, h, wd, c1, c2
    d.Cout, d.KH, d.KW, d.stride = cout, kh, kw, stride
    d.cout_valid = dz.shape[3]
    d.Ho, d.pad_t = same_pad(h, kh, stride)
    d.Wo, d.pad_l = same_pad(wd, kw, stride)
    d.x2_scale = float(x2_scale)
    d.algo = _auto(_AUTO_ALGO[PRECISION]) if WINOGRAD or PRECISION != "fp32" else ALGO_MFMA
    if tuple(dz.shape[:3]) != (n, d.Ho, d.Wo) or dz.shape[3] > cout:
        raise ValueError("conv2d_dgrad: dz shape %s does not match the forward output" % (tuple(dz.shape),))
    nws = int(lib.shdr_conv2d_dgrad_workspace_bytes_f32(ctypes.byref(d), int(which)))
    if nws < 0:
        raise ValueError("conv2d_dgrad: bad descriptor")
    ws = torch.empty(max(nws, 16), device=dz.device, dtype=torch.uint8)
    dx = torch.empty(tuple(x_shape), device=dz.device, dtype=torch.float32)
    # range slots (a chain conv <- activation <- conv of a backward pass never measures: |act' dz| <= |dz|, _carry_range)
    zr = _range_of(dz_in)
    xr = _new_slot(dz.device) if int(lib.shdr_conv2d_dgrad_tracks_range_f32(ctypes.byref(d), int(which))) else None
    if zr is None and xr is not None:
        RANGE_MISSES[("dgrad", tuple(dz.shape), tuple(w.shape))] += 1
    _lib.check(lib.shdr_conv2d_dgrad_ranged_f32(ctypes.byref(d), int(which), _ptr(dz), _ptr(w), _ptr(dx), _ptr(ws), _ptr(zr), _ptr(xr), _stream()),
               "shdr_conv2d_dgrad_ranged_f32")
    if xr is not None:
        _set_range(dx, xr)
    return dx


def soft_hist_bwd(img, dy, max_bin):
    lib = _lib.load()
    img, dy = _chk(_d(img), "img"), _chk(_d(dy), "dy")
    c = img.shape[-1]
    dx = torch.empty_like(img)
    _lib.check(lib.shdr_soft_hist_bwd_f32(_ptr(img), _ptr(dy), _ptr(dx), img.numel() // c, c, int(max_bin), _stream()), "shdr_soft_hist_bwd_f32")
    return dx


def _nhwc_op(fn_name, x, out_shape):
    lib = _lib.load()
    x_in = x
    if _is_h(x):                       # the _f16 twin (csrc/elem_f16.hip)
        x = _chkh(_d(x), "x")
        fn_name = fn_name[:-4] + "_f16"
    else:
        x = _chk(_d(x), "x")
    n, h, w, c = x.shape
    y = torch.empty(out_shape, device=x.device, dtype=x.dtype)
    rc = getattr(lib, fn_name)(_ptr(x), _ptr(y), n, h, w, c, _stream())
    _lib.check(rc, fn_name)
    return _carry_range(y, x_in)        # pooling / bilinear resize: bounded by the input's maximum


def avgpool2(x):
    if _needs_grad(x):
        return AUTOGRAD.avgpool2(x)
    n, h, w, c = x.shape
    return _nhwc_op("shdr_avgpool2_fwd_f32", x, (n, h // 2, w // 2, c))


def maxpool2(x):
    if _needs_grad(x):
        return AUTOGRAD.maxpool2(x)
    n, h, w, c = x.shape
    return _nhwc_op("shdr_maxpool2_fwd_f32", x, (n, h // 2, w // 2, c))


def maxpool3s2(x):
    if _needs_grad(x):
        return AUTOGRAD.maxpool3s2(x)
    n, h, w, c = x.shape
    return _nhwc_op("shdr_maxpool3s2_fwd_f32", x, (n, same_pad(h, 3, 2)[0], same_pad(w, 3, 2)[0], c))


def resize2x(x):
    if _needs_grad(x):
        return AUTOGRAD.resize2x(x)
    n, h, w, c = x.shape
    return _nhwc_op("shdr_resize2x_fwd_f32", x, (n, 2 * h, 2 * w, c))


def global_avg_pool(x):
    if _needs_grad(x):
        return AUTOGRAD.global_avg_pool(x)
    lib = _lib.load()
    n, h, w, c = x.shape
    y = torch.empty((n, c), device=x.device, dtype=torch.float32)
    if _is_h(x):
        _lib.check(lib.shdr_gap_fwd_f16(_ptr(_chkh(_d(x), "x")), _ptr(y), n, h * w, c, _stream()), "shdr_gap_fwd_f16")
        return y
    x = _chk(_d(x), "x")
    _lib.check(lib.shdr_gap_fwd_f32(_ptr(x), _ptr(y), n, h * w, c, _stream()), "shdr_gap_fwd_f32")
    return y


def soft_hist(img, max_bin):
    """linearization_net.py:336-350 on [..., C] tensors -> [..., max_bin*C]."""
    lib = _lib.load()
    img = _chk(_d(img), "img")
    c = img.shape[-1]
    npix = img.numel() // c
    y = torch.empty(tuple(img.shape[:-1]) + (int(max_bin) * c,), device=img.device, dtype=torch.float32)
    _lib.check(lib.shdr_soft_hist_fwd_f32(_ptr(img), _ptr(y), npix, c, int(max_bin), _stream()),
               "shdr_soft_hist_fwd_f32")
    return y


def lin_frontend(img, channels=96, dtype=None):
    """dtype: torch.float16 inside precision("fp16") (native-fp16 feature maps), float32 otherwise"""
    dtype = dtype or (HALF if native_fp16() else torch.float32)
    if _needs_grad(img):
        return AUTOGRAD.lin_frontend(img, channels, dtype)
    lib = _lib.load()
    img_in = img
    img = _chk(_d(img), "img")
    n, h, w, c = img.shape
    if c != 3:
        raise ValueError("lin_frontend: expected 3 channels, got %d" % c)
    y = torch.empty((n, h, w, channels), device=img.device, dtype=dtype)
    fn = "shdr_lin_frontend_fwd_f16" if dtype == HALF else "shdr_lin_frontend_fwd_f32"
    _lib.check(getattr(lib, fn)(_ptr(img), _ptr(y), n, h, w, channels, _stream()), fn)
    b = _bound_of(img_in)              # image: b, sobel: sum |coefficient| = 8 times b, soft-histogram channels: [0, 1]
    return y if b is None else set_bound(y, max(1.0, 8.0 * b))


def invcrf_decode(feat, wfc, bfc, table):
    if _needs_grad(feat, wfc, bfc):
        return AUTOGRAD.invcrf_decode(feat, wfc, bfc, table)
    lib = _lib.load()
    feat, wfc, bfc, table = (_chk(_d(t), nm) for t, nm in
                             ((feat, "feat"), (wfc, "wfc"), (bfc, "bfc"), (table, "table")))
    b, f = feat.shape
    k = table.shape[0]
    if tuple(wfc.shape) != (f, 11) or bfc.numel() != 11 or tuple(table.shape) != (k, 12):
        raise ValueError("invcrf_decode: expected wfc [F,11], bfc [11], table [K,12]")
    out = torch.empty((b, k), device=feat.device, dtype=torch.float32)
    _lib.check(lib.shdr_invcrf_decode_fwd_f32(_ptr(feat), _ptr(wfc), _ptr(bfc), _ptr(table), _ptr(out),
                                              b, f, k, _stream()), "shdr_invcrf_decode_fwd_f32")
    return out


def increase(rf):
    if _needs_grad(rf):
        return AUTOGRAD.increase(rf)
    lib = _lib.load()
    rf = _chk(_d(rf), "rf")
    b, k = rf.shape
    out = torch.empty_like(rf)
    _lib.check(lib.shdr_increase_fwd_f32(_ptr(rf), _ptr(out), b, k, _stream()), "shdr_increase_fwd_f32")
    return out


def apply_rf(x, rf):
    if _needs_grad(x, rf):
        return AUTOGRAD.apply_rf(x, rf)
    lib = _lib.load()
    x = _chk(_d(x), "x")
    rf = _chk(_d(rf), "rf")
    b = x.shape[0]
    if rf.shape[0] != b:
        raise ValueError("apply_rf: batch mismatch %d vs %d" % (b, rf.shape[0]))
    y = torch.empty_like(x)
    _lib.check(lib.shdr_apply_rf_fwd_f32(_ptr(x), _ptr(rf), _ptr(y), b, x.numel() // b, rf.shape[1],
                                         _stream()), "shdr_apply_rf_fwd_f32")
    return y


def clip(x, lo, hi):
    if _needs_grad(x):
        return AUTOGRAD.clip(x, lo, hi)
    lib = _lib.load()
    x = _chk(_d(x), "x")
    y = torch.empty_like(x)
    _lib.check(lib.shdr_clip_fwd_f32(_ptr(x), _ptr(y), x.numel(), float(lo), float(hi), _stream()),
               "shdr_clip_fwd_f32")
    return set_bound(y, max(abs(float(lo)), abs(float(hi))))


def logc(x):
    if _needs_grad(x):
        return AUTOGRAD.logc(x)
    lib = _lib.load()
    x = _chk(_d(x), "x")
    y = torch.empty_like(x)
    _lib.check(lib.shdr_logc_fwd_f32(_ptr(x), _ptr(y), x.numel(), _stream()), "shdr_logc_fwd_f32")
    return y


def _pix3(x, name):
    x = _chk(_d(x), name)
    if x.shape[-1] != 3:
        raise ValueError("%s: expected 3 channels, got %d" % (name, x.shape[-1]))
    return x, x.numel() // 3


def vgg_preprocess(x, out_channels=3, dtype=torch.float32):
    """x*255, RGB->BGR, minus VGG mean; out_channels=4 appends a zero channel (MFMA-friendly); dtype float16: the zero-padded
    fp16 feature map of the native-fp16 path (out_channels % 8 == 0)."""
    if _needs_grad(x):
        return AUTOGRAD.vgg_preprocess(x, out_channels, dtype)
    lib = _lib.load()
    x_in = x
    x, npix = _pix3(x, "x")
    if dtype == HALF:
        y = torch.empty(tuple(x.shape[:-1]) + (out_channels,), device=x.device, dtype=HALF)
        _lib.check(lib.shdr_pack3_f16(_ptr(x), None, None, None, 1, _ptr(y), out_channels, npix, 1, _stream()), "shdr_pack3_f16")
        return y
    y = torch.empty(tuple(x.shape[:-1]) + (out_channels,), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_vgg_preprocess_fwd_f32(_ptr(x), _ptr(y), npix, out_channels, _stream()),
               "shdr_vgg_preprocess_fwd_f32")
    b = _bound_of(x_in)
    return y if b is None else set_bound(y, 255.0 * b + 124.0)     # x * 255 - mean, |mean| < 124


def reverse3(x):
    if _needs_grad(x):
        return AUTOGRAD.reverse3(x)
    lib = _lib.load()
    x, npix = _pix3(x, "x")
    y = torch.empty_like(x)
    _lib.check(lib.shdr_reverse3_fwd_f32(_ptr(x), _ptr(y), npix, _stream()), "shdr_reverse3_fwd_f32")
    return y


def alpha_blend(b_pred, hal_bgr, thr=0.12, return_alpha=False):
    if _needs_grad(b_pred, hal_bgr):
        if return_alpha:
            raise NotImplementedError("alpha_blend: return_alpha is not available on the taped path")
        return AUTOGRAD.alpha_blend(b_pred, hal_bgr, thr)
    lib = _lib.load()
    b_pred, npix = _pix3(b_pred, "b_pred")
    hal_bgr, npix2 = _pix3(hal_bgr, "hal_bgr")
    if npix != npix2:
        raise ValueError("alpha_blend: shape mismatch")
    a = torch.empty_like(b_pred)
    alpha = torch.empty(tuple(b_pred.shape[:-1]) + (1,), device=a.device, dtype=torch.float32) if return_alpha else None
    _lib.check(lib.shdr_alpha_blend_fwd_f32(_ptr(b_pred), _ptr(hal_bgr), _ptr(a), _ptr(alpha), npix,
                                            float(thr), _stream()), "shdr_alpha_blend_fwd_f32")
    return (a, alpha) if return_alpha else a


def pack3(srcs, out_channels=None, dtype=torch.float32):
    if _needs_grad(*srcs):
        return AUTOGRAD.pack3(list(srcs), out_channels, dtype)
    lib = _lib.load()
    srcs_in = list(srcs)
    srcs = [_pix3(s, "src%d" % i)[0] for i, s in enumerate(srcs)]
    n = len(srcs)
    if not 1 <= n <= 4:
        raise ValueError("pack3: 1..4 sources")
    if any(s.shape != srcs[0].shape for s in srcs):
        raise ValueError("pack3: shape mismatch")
    oc = out_channels or 3 * n
    y = torch.empty(tuple(srcs[0].shape[:-1]) + (oc,), device=srcs[0].device, dtype=dtype)
    p = [_ptr(s) for s in srcs] + [None] * (4 - n)
    if dtype == HALF:
        _lib.check(lib.shdr_pack3_f16(p[0], p[1], p[2], p[3], n, _ptr(y), oc, srcs[0].numel() // 3, 0, _stream()), "shdr_pack3_f16")
        return y
    _lib.check(lib.shdr_pack3_fwd_f32(p[0], p[1], p[2], p[3], n, _ptr(y), oc, srcs[0].numel() // 3,
                                      _stream()), "shdr_pack3_fwd_f32")
    if n == 1:                               # a channel-padded copy: the same range
        return _carry_range(y, srcs_in[0])
    bounds = [_bound_of(t) for t in srcs_in]      # (device-side slots of several sources are not merged: measured by the consumer)
    return y if None in bounds else set_bound(y, max(bounds))


# ---------------------------------------------------------------------------
# raw wrappers of the backward / training kernels (no autograd; see _autograd.py)
# ---------------------------------------------------------------------------
def _conv_desc(x_shape, w_shape, stride, c2, x2_scale, cout_valid):
    n, h, wd, c1 = x_shape
    kh, kw, cin, cout_gemm = w_shape
    ho, pt = same_pad(h, kh, stride)
    wo, pl = same_pad(wd, kw, stride)
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C1, d.C2 = n, h, wd, c1, c2
    d.Cout, d.KH, d.KW, d.stride = cout_gemm, kh, kw, stride
    d.cout_valid = cout_valid or cout_gemm
    d.pad_t, d.pad_l, d.Ho, d.Wo = pt, pl, ho, wo
    d.x2_scale = float(x2_scale)
    return d


def pad_channels(x, channels):
    """zero-pad the channel axis to `channels` (no-op if already that wide)"""
    lib = _lib.load()
    x = _chk(_d(x), "x")
    c = x.shape[-1]
    if c == channels:
        return x
    y = torch.empty(tuple(x.shape[:-1]) + (channels,), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_pad_channels_f32(_ptr(x), _ptr(y), x.numel() // c, c, channels, _stream()), "shdr_pad_channels_f32")
    return y


def _up16(c):
    return (c + 15) // 16 * 16


WGRAD_X3_MIN_CH = 128     # conv2d_wgrad: layers with at least this many channels per source and output channels take the split-operand kernel


def _split_planes(lib, t, slot):
    """(high plane, low plane, range slot) of an fp32 tensor for the split-operand weight gradient; the range is measured when the
    tensor carries no slot (output gradients never do)"""
    if slot is None:
        RANGE_MISSES[("wgrad operand", tuple(t.shape))] += 1
        slot = _new_slot(t.device)
        _lib.check(lib.shdr_absmax_f32(_ptr(t), t.numel(), _ptr(slot), _stream()), "shdr_absmax_f32")
    hi = torch.empty(t.shape, device=t.device, dtype=torch.float16)
    lo = torch.empty(t.shape, device=t.device, dtype=torch.float16)
    _lib.check(lib.shdr_x3_split_planes_f32(_ptr(t), t.numel(), _ptr(slot), _ptr(hi), _ptr(lo), _stream()), "shdr_x3_split_planes_f32")
    return hi, lo, slot


def conv2d_wgrad(x, x2, dz, w_shape, stride=1, x2_scale=1.0, out=None):
    """dW [kh,kw,C1+C2,Cout] of conv(concat[x, x2_scale*x2], W) given dz = dL/d(conv output).

    Channel counts that are not multiples of 16 (3/4-channel images, 3-channel heads) are zero-padded so
    that the layer runs on the MFMA weight-gradient tiles; the true rows / columns are sliced out.
    `out`: a gradient buffer of shape w_shape to ACCUMULATE into (the kernels add with atomics anyway): no zero fill and no
    separate add -- used for variables whose .grad is a view of the flat gradient buffer (pipeline.FlatParams).
    Under `deterministic(True)` every family runs its slab form and the fold writes out = out + S WITHOUT an atomic: the caller orders the
    call against every other writer of `out` (one stream per gradient range: DESIGN.md "Deterministic mode")."""
    kh, kw, cin, cout = w_shape
    c1 = x.shape[3]
    c2 = 0 if x2 is None else x2.shape[3]
    if out is not None and (tuple(out.shape) != tuple(w_shape) or not out.is_contiguous() or out.dtype != torch.float32):
        raise ValueError("conv2d_wgrad: out must be a contiguous float32 tensor of shape %s" % (tuple(w_shape),))
    if c1 % 16 or c2 % 16 or cout % 16:
        if out is not None:
            out.add_(conv2d_wgrad(x, x2, dz, w_shape, stride, x2_scale))      # padded layers: sliced result, parameter-sized add
            return out
        c1p, c2p, coutp = _up16(c1), (_up16(c2) if c2 else 0), _up16(cout)
        dwp = conv2d_wgrad(pad_channels(x, c1p), None if x2 is None else pad_channels(x2, c2p), pad_channels(dz, coutp),
                           (kh, kw, c1p + c2p, coutp), stride, x2_scale)
        if c2:
            return torch.cat([dwp[:, :, :c1, :cout], dwp[:, :, c1p:c1p + c2, :cout]], dim=2).contiguous()
        return dwp[:, :, :c1, :cout].contiguous()
    lib = _lib.load()
    x_in, x2_in, dz_in = x, x2, dz
    x, dz = _chk(_d(x), "x"), _chk(_d(dz), "dz")
    if x2 is not None:
        _chk(_d(x2), "x2")
    if DETERMINISTIC and PRECISION != "fp32":
        raise ValueError("conv2d_wgrad: the deterministic mode covers precision 'fp32' only, not %r" % (PRECISION,))
    # Deep k x k layers (>= WGRAD_X3_MIN_CH channels on both sides): the split-operand weight gradient on the fp16 matrix pipe
    # (csrc/wgrad_x3.hip) -- one split pass per tensor, then three fp16 MFMAs per operand pair.  Measured at batch 32 (tools/wgrad_x3_bench.py,
    # split passes included) against the Winograd-domain fp32 kernel: 512 -> 512 at 32^2 0.85 -> 0.60 ms, 512 -> 256 at 64^2 1.61 -> 1.06,
    # 256 -> 256 at 64^2 0.85 -> 0.62, 256 -> 128 at 128^2 1.59 -> 1.27, 128 -> 128 at 128^2 0.78 -> 0.72 (215-290 TFLOP/s in fp32 layer
    # FLOPs); 1x1 layers do too little arithmetic per element for the two split passes (0.33 -> 0.43 ms at 256 + 256 -> 256) and stay exact
    # (a 7x7 layer does 49 taps of arithmetic per split element: the stem of the Linearization-Net, 96 -> 64, 3.0 -> 1.9 ms at 32 x 256^2, split passes included)
    wide = min(c1, c2 or c1, cout) >= WGRAD_X3_MIN_CH or (kh * kw >= 25 and min(c1, c2 or c1, cout) >= 64)
    if (PRECISION == "fp32" and not EXACT_FP32 and WINOGRAD and kh * kw >= 9 and wide and cin == c1 + c2
            and cout == dz.shape[3] and x.numel() % 8 == 0 and dz.numel() % 8 == 0 and (x2 is None or x2.numel() % 8 == 0)):
        d = _conv_desc(x.shape, w_shape, stride, c2, x2_scale, None)
        if tuple(dz.shape[:3]) == (x.shape[0], d.Ho, d.Wo) and all(int(lib.shdr_conv2d_wgrad_x3_ok_f32(ctypes.byref(d), i)) for i in range(2 if c2 else 1)):
            dw = out if out is not None else torch.zeros(tuple(w_shape), device=x.device, dtype=torch.float32)
            zh, zl, zr = _split_planes(lib, dz, _range_of(dz_in))
            _set_range(dz_in, zr)           # the input gradient of the same layer (called next) takes the slot instead of measuring again
            for src, src_in, which in ((x, x_in, 0),) + (((_d(x2), x2_in, 1),) if x2 is not None else ()):
                xh, xl, xr = _split_planes(lib, src, _range_of(src_in))
                if DETERMINISTIC:
                    ws, nws = _det_ws(_lib.DET_CONV2D_WGRAD_X3, x.device, d=d, c=which)
                    _lib.check(lib.shdr_conv2d_wgrad_x3_det_f32(ctypes.byref(d), _ptr(xh), _ptr(xl), which, _ptr(zh), _ptr(zl), _ptr(xr), _ptr(zr),
                                                                _ptr(dw), _ptr(ws), nws, _stream()), "shdr_conv2d_wgrad_x3_det_f32")
                    continue
                _lib.check(lib.shdr_conv2d_wgrad_x3_f32(ctypes.byref(d), _ptr(xh), _ptr(xl), which, _ptr(zh), _ptr(zl), _ptr(xr), _ptr(zr),
                                                        _ptr(dw), _stream()), "shdr_conv2d_wgrad_x3_f32")
            return dw
    # (in the reduced-precision modes too for <= 64 channels per source: the exact Winograd-domain kernel is faster there than the
    #  fp16-operand kernel -- 16 x 512^2 x 64 -> 64: 1.77 vs 2.98 ms -- and errs on the accurate side)
    if (WINOGRAD and (PRECISION == "fp32" or max(c1, c2) <= 64) and (kh, kw) == (3, 3) and stride == 1 and c1 % 32 == 0 and c2 % 32 == 0
            and cout % 64 == 0 and cin == c1 + c2 and cout == dz.shape[3] and tuple(dz.shape[:3]) == tuple(x.shape[:3])):
        # Winograd-domain weight gradient (csrc/wgrad_winograd.hip): 2.25x fewer MFMAs than the direct form
        n, h, w, _ = x.shape
        dw = out if out is not None else torch.zeros(tuple(w_shape), device=x.device, dtype=torch.float32)
        for src, cx, off, sc in ((x, c1, 0, 1.0),) + (((_d(x2), c2, c1, float(x2_scale)),) if x2 is not None else ()):
            du = torch.empty((16, cx, cout), device=x.device, dtype=torch.float32)       # scratch, zeroed by the library call
            if DETERMINISTIC:
                dd = _conv_desc(x.shape, w_shape, stride, c2, x2_scale, None)
                ws, nws = _det_ws(_lib.DET_CONV2D_WGRAD_WINOGRAD, x.device, d=dd, c=1 if off else 0)
                _lib.check(lib.shdr_conv2d_wgrad_winograd_det_f32(_ptr(src), _ptr(dz), _ptr(du), _ptr(dw), _ptr(ws), nws, n, h, w, cx, cout, cin,
                                                                  off, sc, _stream()), "shdr_conv2d_wgrad_winograd_det_f32")
                continue
            _lib.check(lib.shdr_conv2d_wgrad_winograd_f32(_ptr(src), _ptr(dz), _ptr(du), _ptr(dw), n, h, w, cx, cout, cin, off, sc,
                                                          _stream()), "shdr_conv2d_wgrad_winograd_f32")
        return dw
    if cin != x.shape[3] + c2 or cout != dz.shape[3]:
        raise ValueError("conv2d_wgrad: filter %s does not match x %s (+%d) / dz %s"
                         % (tuple(w_shape), tuple(x.shape), c2, tuple(dz.shape)))
    d = _conv_desc(x.shape, w_shape, stride, c2, x2_scale, None)
    d.algo = _AUTO_ALGO[PRECISION]
    if tuple(dz.shape[:3]) != (x.shape[0], d.Ho, d.Wo):
        raise ValueError("conv2d_wgrad: dz spatial shape mismatch")
    dw = out if out is not None else torch.zeros(tuple(w_shape), device=x.device, dtype=torch.float32)
    if DETERMINISTIC:
        for src, which in ((x, 0),) + (((_chk(_d(x2), "x2"), 1),) if x2 is not None else ()):
            ws, nws = _det_ws(_lib.DET_CONV2D_WGRAD, x.device, d=d, c=which)
            _lib.check(lib.shdr_conv2d_wgrad_det_f32(ctypes.byref(d), _ptr(src), which, _ptr(dz), _ptr(dw), _ptr(ws), nws, _stream()),
                       "shdr_conv2d_wgrad_det_f32")
        return dw
    _lib.check(lib.shdr_conv2d_wgrad_f32(ctypes.byref(d), _ptr(x), 0, _ptr(dz), _ptr(dw), _stream()), "shdr_conv2d_wgrad_f32")
    if x2 is not None:
        _lib.check(lib.shdr_conv2d_wgrad_f32(ctypes.byref(d), _ptr(_d(x2)), 1, _ptr(dz), _ptr(dw), _stream()),
                   "shdr_conv2d_wgrad_f32")
    return dw


def filter_transform(w, c_begin, c_count, scale=1.0):
    """wt[kh,kw,co,ci] = scale * w[KH-1-kh, KW-1-kw, c_begin+ci, co]: the dgrad filter."""
    lib = _lib.load()
    w = _chk(_d(w), "w")
    kh, kw, cin, cout = w.shape
    wt = torch.empty((kh, kw, cout, c_count), device=w.device, dtype=torch.float32)
    _lib.check(lib.shdr_filter_transform_f32(_ptr(w), _ptr(wt), kh, kw, cin, cout, c_begin, c_count, float(scale), _stream()),
               "shdr_filter_transform_f32")
    return wt


def bias_grad(dz, out=None):
    lib = _lib.load()
    dz = _chk(_d(dz), "dz")
    c = dz.shape[-1]
    db = out if out is not None else torch.zeros(c, device=dz.device, dtype=torch.float32)
    if DETERMINISTIC:
        ws, nws = _det_ws(_lib.DET_BIAS_GRAD, dz.device, n=dz.numel() // c, c=c)
        _lib.check(lib.shdr_bias_grad_det_f32(_ptr(dz), _ptr(db), _ptr(ws), nws, dz.numel() // c, c, _stream()), "shdr_bias_grad_det_f32")
        return db
    _lib.check(lib.shdr_bias_grad_f32(_ptr(dz), _ptr(db), dz.numel() // c, c, _stream()), "shdr_bias_grad_f32")
    return db


def _bias_ws(c, device):
    """one row of partial channel sums per reduction block of act_bwd_bias (sized by the library)"""
    return torch.empty(int(_lib.load().shdr_workspace_bytes(_lib.OP_ACT_BWD_BIAS, None, int(c))) // 4, device=device, dtype=torch.float32)


def act_bwd_bias(dy, y, act, out=None):
    """(dz, db) of y = act(z + bias): dz = dy * act'(y), db = sum over pixels of dz -- one fused pass when the channel
    count allows (C / 4 a power of two), the act_bwd + bias_grad pair otherwise.  `out`: gradient buffer to accumulate db into."""
    if _is_h(dy):
        return act_bwd_bias_h(dy, y, act, True, out)
    dy_in = dy
    dy = _chk(_d(dy), "dy")
    c = dy.shape[-1]
    q = c // 4
    if c % 4 or q > 256 or q & (q - 1):
        dz = act_bwd(dy_in, y, act) if act != ACT_NONE else dy_in
        return dz, bias_grad(dz, out)
    lib = _lib.load()
    db = out if out is not None else torch.zeros(c, device=dy.device, dtype=torch.float32)
    if act == ACT_NONE:
        dz, yp, zp = dy_in, None, None  # (the caller's tensor object: it carries the range slot)
    else:
        y = _chk(_d(y), "y")
        dz = torch.empty_like(dy)
        yp, zp = _ptr(y), _ptr(dz)
    fn = "shdr_act_bwd_bias_det_f32" if DETERMINISTIC else "shdr_act_bwd_bias_f32"
    _lib.check(getattr(lib, fn)(_ptr(dy), yp, zp, _ptr(db), _ptr(_bias_ws(c, dy.device)), dy.numel() // c, c, act, _stream()), fn)
    if dz is not dy_in:
        _carry_range(dz, dy_in)         # |act'(y)| <= 1
    return dz, db


def act_bwd(dy, y, act):
    if _is_h(dy):
        return act_bwd_bias_h(dy, y, act, False)[0]
    lib = _lib.load()
    dy_in = dy
    dy, y = _chk(_d(dy), "dy"), _chk(_d(y), "y")
    dx = torch.empty_like(dy)
    _lib.check(lib.shdr_act_bwd_f32(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), act, _stream()), "shdr_act_bwd_f32")
    return _carry_range(dx, dy_in)     # |act'(y)| <= 1 for relu / leaky relu / tanh


def clip_bwd(dy, x, lo, hi):
    lib = _lib.load()
    dy_in = dy
    dy, x = _chk(_d(dy), "dy"), _chk(_d(x), "x")
    dx = torch.empty_like(dy)
    _lib.check(lib.shdr_clip_bwd_f32(_ptr(dy), _ptr(x), _ptr(dx), dy.numel(), float(lo), float(hi), _stream()), "shdr_clip_bwd_f32")
    return _carry_range(dx, dy_in)


def add(a, b, relu=False):
    """a + b (relu: max(a + b, 0), fp16 feature maps only)"""
    if _needs_grad(a, b):
        if relu:
            return AUTOGRAD.add_relu(a, b)
        return AUTOGRAD.add(a, b)
    lib = _lib.load()
    if _is_h(a):
        a, b = _chkh(_d(a), "a"), _chkh(_d(b), "b")
        if a.shape != b.shape:
            raise ValueError("add: shape mismatch")
        y = torch.empty_like(a)
        _lib.check(lib.shdr_add_f16(_ptr(a), _ptr(b), _ptr(y), a.numel(), int(bool(relu)), _stream()), "shdr_add_f16")
        return y
    if relu:
        s = add(a, b)
        return _carry_range(clip(s, 0.0, float("inf")), s)     # R4
    a, b = _chk(_d(a), "a"), _chk(_d(b), "b")
    if a.shape != b.shape:
        raise ValueError("add: shape mismatch")
    y = torch.empty_like(a)
    yr = _new_slot(a.device)            # max |a + b| out of the same pass (a gradient sum usually feeds a split-operand dgrad / wgrad)
    _lib.check(lib.shdr_add_ranged_f32(_ptr(a), _ptr(b), _ptr(y), a.numel(), _ptr(yr), _stream()), "shdr_add_ranged_f32")
    return _set_range(y, yr)


def mark(x, callback):
    """x itself; on a gradient tape `callback()` runs when the backward pass reaches this point (every backward op of the layers AFTER
    it in the forward has been enqueued): where the data-parallel steps launch a gradient bucket's all-reduce"""
    if callback is None or not _needs_grad(x):
        return x
    return _carry_range(AUTOGRAD.mark(x, callback), x)


def fork(x, n=2):
    """n aliases of x for n consumers (skip connections, residual shortcuts, multi-term losses): on a gradient tape the consumers'
    gradients are summed by the add kernel of this library; without a tape it is x itself, n times"""
    if not _needs_grad(x):
        return (x,) * n
    return tuple(_carry_range(t, x) for t in AUTOGRAD.fork(x, n))      # (the aliases are new tensor objects: hand the range slot on)


def affine_act(x, scale=None, shift=None, residual=None, act=ACT_NONE):
    """act(x * scale[c] + shift[c] + residual) on NHWC"""
    if _needs_grad(x, scale, shift, residual):
        return AUTOGRAD.affine_act(x, scale, shift, residual, act)
    lib = _lib.load()
    x = _chk(_d(x), "x")
    c = x.shape[-1]
    for t, nm in ((scale, "scale"), (shift, "shift")):
        if t is not None and _chk(_d(t), nm).numel() != c:
            raise ValueError("affine_act: %s must have %d elements" % (nm, c))
    if residual is not None and _chk(_d(residual), "residual").shape != x.shape:
        raise ValueError("affine_act: residual shape %s != %s" % (tuple(residual.shape), tuple(x.shape)))
    y = torch.empty_like(x)
    _lib.check(lib.shdr_affine_act_f32(_ptr(x), _ptr(_d(scale)), _ptr(_d(shift)), _ptr(_d(residual)), _ptr(y), x.numel() // c, c,
                                       act, _stream()), "shdr_affine_act_f32")
    return y


def _bwd_nhwc(fn_name, x_shape, *tensors):
    """input-gradient kernels taking (tensors..., dx, N, H, W, C) of the op's INPUT shape"""
    lib = _lib.load()
    if _is_h(tensors[0]):
        ts = [_chkh(_d(t), "t%d" % i) for i, t in enumerate(tensors)]
        fn_name = fn_name[:-4] + "_f16"
    else:
        ts = [_chk(_d(t), "t%d" % i) for i, t in enumerate(tensors)]
    n, h, w, c = x_shape
    dx = torch.empty(tuple(x_shape), device=ts[0].device, dtype=ts[0].dtype)
    _lib.check(getattr(lib, fn_name)(*[_ptr(t) for t in ts], _ptr(dx), n, h, w, c, _stream()), fn_name)
    return dx


def avgpool2_bwd(dy, x_shape):
    return _carry_range(_bwd_nhwc("shdr_avgpool2_bwd_f32", x_shape, dy), dy)          # dy / 4


def maxpool2_bwd(x, dy):
    return _carry_range(_bwd_nhwc("shdr_maxpool2_bwd_f32", x.shape, x, dy), dy)       # dy or 0 (disjoint windows)


def maxpool3s2_bwd(x, y, dy):
    """`y` is the forward's output maxpool3s2(x)"""
    return _bwd_nhwc("shdr_maxpool3s2_bwd_f32", x.shape, x, y, dy)


def resize2x_bwd(dy, x_shape):
    if _is_h(dy):
        return _bwd_nhwc("shdr_resize2x_bwd_f32", x_shape, dy)
    lib = _lib.load()
    dy = _chk(_d(dy), "dy")
    n, h, w, c = x_shape
    dx = torch.empty(tuple(x_shape), device=dy.device, dtype=torch.float32)
    xr = _new_slot(dy.device)           # max |dx| out of the same pass (the consumer is the input gradient of the conv in front)
    _lib.check(lib.shdr_resize2x_bwd_ranged_f32(_ptr(dy), _ptr(dx), n, h, w, c, _ptr(xr), _stream()), "shdr_resize2x_bwd_ranged_f32")
    return _set_range(dx, xr)


def upsample_zero2(dy, x_shape):
    return _carry_range(_bwd_nhwc("shdr_upsample_zero2_f32", x_shape, dy), dy)         # dy or 0


def gap_bwd(dy, x_shape, dtype=torch.float32):
    lib = _lib.load()
    dy = _chk(_d(dy), "dy")
    n, h, w, c = x_shape
    dx = torch.empty(tuple(x_shape), device=dy.device, dtype=dtype)
    fn = "shdr_gap_bwd_f16" if dtype == HALF else "shdr_gap_bwd_f32"
    _lib.check(getattr(lib, fn)(_ptr(dy), _ptr(dx), n, h * w, c, _stream()), fn)
    return dx


def _bn_ws(c, device):
    """workspace of the BatchNorm reductions (sums + one partial row per block), sized by the library"""
    nbytes = int(_lib.load().shdr_workspace_bytes(_lib.OP_BATCHNORM, None, int(c)))
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64)


def bn_stats(x, moving_mean=None, moving_var=None, momentum=0.99):
    """batch mean / biased variance over (N,H,W); optionally updates the moving statistics in place."""
    lib = _lib.load()
    h = _is_h(x)
    x = _chkh(_d(x), "x") if h else _chk(_d(x), "x")
    c = x.shape[-1]
    mean = torch.empty(c, device=x.device, dtype=torch.float32)
    var = torch.empty(c, device=x.device, dtype=torch.float32)
    ws = _bn_ws(c, x.device)
    if h:
        _no_det_h("bn_stats")
    fn = "shdr_bn_stats_f16" if h else ("shdr_bn_stats_det_f32" if DETERMINISTIC else "shdr_bn_stats_f32")
    _lib.check(getattr(lib, fn)(_ptr(x), _ptr(ws), _ptr(mean), _ptr(var), _ptr(_d(moving_mean)), _ptr(_d(moving_var)),
                                x.numel() // c, c, float(momentum), _stream()), fn)
    _mutated(moving_mean, moving_var)
    return mean, var


def bn_train_apply(x, mean, var, gamma, beta, eps, relu):
    lib = _lib.load()
    h = _is_h(x)
    x = _chkh(_d(x), "x") if h else _chk(_d(x), "x")
    c = x.shape[-1]
    y = torch.empty_like(x)
    if not h:                          # fp32: the kernel also writes the range slot of y (its consumer is usually a split-operand conv)
        yr = _new_slot(x.device)
        _lib.check(lib.shdr_bn_train_apply_ranged_f32(_ptr(x), _ptr(mean), _ptr(var), _ptr(_d(gamma)), _ptr(_d(beta)), _ptr(y),
                                                      x.numel() // c, c, float(eps), int(bool(relu)), _ptr(yr), _stream()),
                   "shdr_bn_train_apply_ranged_f32")
        return _set_range(y, yr)
    _lib.check(lib.shdr_bn_train_apply_f16(_ptr(x), _ptr(mean), _ptr(var), _ptr(_d(gamma)), _ptr(_d(beta)), _ptr(y),
                                           x.numel() // c, c, float(eps), int(bool(relu)), _stream()), "shdr_bn_train_apply_f16")
    return y


def bn_bwd(dy, x, y_relu, mean, var, gamma, eps, dgamma_out=None, dbeta_out=None):
    """(dx, dgamma, dbeta); dgamma_out / dbeta_out: gradient buffers to accumulate into instead of fresh zero tensors"""
    lib = _lib.load()
    h = _is_h(x)
    dy, x = (_chkh(_d(dy), "dy"), _chkh(_d(x), "x")) if h else (_chk(_d(dy), "dy"), _chk(_d(x), "x"))
    c = x.shape[-1]
    dgamma = dgamma_out if dgamma_out is not None else torch.zeros(c, device=x.device, dtype=torch.float32)
    dbeta = dbeta_out if dbeta_out is not None else torch.zeros(c, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    ws = _bn_ws(c, x.device)
    if h:
        _no_det_h("bn_bwd")
        _lib.check(lib.shdr_bn_bwd_f16(_ptr(dy), _ptr(x), _ptr(_d(y_relu)), _ptr(mean), _ptr(var), _ptr(_d(gamma)), _ptr(ws),
                                       _ptr(dgamma), _ptr(dbeta), _ptr(dx), x.numel() // c, c, float(eps), _stream()), "shdr_bn_bwd_f16")
        return dx, dgamma, dbeta
    xr = _new_slot(x.device)            # max |dx| out of the apply pass (the consumer is the input / weight gradient of the conv in front)
    fn = "shdr_bn_bwd_ranged_det_f32" if DETERMINISTIC else "shdr_bn_bwd_ranged_f32"
    _lib.check(getattr(lib, fn)(_ptr(dy), _ptr(x), _ptr(_d(y_relu)), _ptr(mean), _ptr(var), _ptr(_d(gamma)), _ptr(ws),
                                _ptr(dgamma), _ptr(dbeta), _ptr(dx), x.numel() // c, c, float(eps), _ptr(xr), _stream()), fn)
    return _set_range(dx, xr), dgamma, dbeta


def invcrf_decode_bwd(dinv, feat, wfc, table):
    lib = _lib.load()
    dinv, feat, wfc, table = (_chk(_d(t), "t") for t in (dinv, feat, wfc, table))
    b, f = feat.shape
    k = table.shape[0]
    dfeat = torch.empty_like(feat)
    dwfc = torch.zeros_like(wfc)
    dbfc = torch.zeros(11, device=feat.device, dtype=torch.float32)
    if DETERMINISTIC:
        ws, nws = _det_ws(_lib.DET_INVCRF_DECODE_BWD, feat.device, c=b, k=f)
        _lib.check(lib.shdr_invcrf_decode_bwd_det_f32(_ptr(dinv), _ptr(feat), _ptr(wfc), _ptr(table), _ptr(dfeat), _ptr(dwfc), _ptr(dbfc),
                                                      _ptr(ws), nws, b, f, k, _stream()), "shdr_invcrf_decode_bwd_det_f32")
        return dfeat, dwfc, dbfc
    _lib.check(lib.shdr_invcrf_decode_bwd_f32(_ptr(dinv), _ptr(feat), _ptr(wfc), _ptr(table), _ptr(dfeat), _ptr(dwfc),
                                              _ptr(dbfc), b, f, k, _stream()), "shdr_invcrf_decode_bwd_f32")
    return dfeat, dwfc, dbfc


def increase_bwd(rf, dout):
    lib = _lib.load()
    rf, dout = _chk(_d(rf), "rf"), _chk(_d(dout), "dout")
    b, k = rf.shape
    drf = torch.empty_like(rf)
    _lib.check(lib.shdr_increase_bwd_f32(_ptr(rf), _ptr(dout), _ptr(drf), b, k, _stream()), "shdr_increase_bwd_f32")
    return drf


def apply_rf_bwd(x, rf, dy, need_dx):
    lib = _lib.load()
    x, rf, dy = _chk(_d(x), "x"), _chk(_d(rf), "rf"), _chk(_d(dy), "dy")
    b = x.shape[0]
    drf = torch.zeros_like(rf)
    dx = torch.empty_like(x) if need_dx else None
    if DETERMINISTIC:
        ws, nws = _det_ws(_lib.DET_APPLY_RF_BWD, x.device, n=x.numel() // b, c=b, k=rf.shape[1])
        _lib.check(lib.shdr_apply_rf_bwd_det_f32(_ptr(x), _ptr(rf), _ptr(dy), _ptr(drf), _ptr(dx), _ptr(ws), nws, b, x.numel() // b,
                                                 rf.shape[1], _stream()), "shdr_apply_rf_bwd_det_f32")
        return drf, dx
    _lib.check(lib.shdr_apply_rf_bwd_f32(_ptr(x), _ptr(rf), _ptr(dy), _ptr(drf), _ptr(dx), b, x.numel() // b, rf.shape[1],
                                         _stream()), "shdr_apply_rf_bwd_f32")
    return drf, dx


def diff_loss(a, b, mode):
    """per-sample mean of (a-b)^2 (mode 0) or |a-b| (mode 1): [B]"""
    if _needs_grad(a, b):
        return AUTOGRAD.diff_loss(a, b, mode)
    lib = _lib.load()
    a, b = _chk(_d(a), "a"), _chk(_d(b), "b")
    if a.shape != b.shape:
        raise ValueError("diff_loss: shape mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    bs = a.shape[0]
    out = torch.empty(bs, device=a.device, dtype=torch.float32)
    if DETERMINISTIC:
        ws, nws = _det_ws(_lib.DET_DIFF_LOSS, a.device, n=a.numel() // bs, c=bs)
        _lib.check(lib.shdr_diff_loss_det_f32(_ptr(a), _ptr(b), _ptr(out), _ptr(ws), nws, bs, a.numel() // bs, mode, _stream()),
                   "shdr_diff_loss_det_f32")
        return out
    _lib.check(lib.shdr_diff_loss_f32(_ptr(a), _ptr(b), _ptr(out), bs, a.numel() // bs, mode, _stream()), "shdr_diff_loss_f32")
    return out


def diff_loss_bwd(a, b, g, mode):
    lib = _lib.load()
    a, b, g = _chk(_d(a), "a"), _chk(_d(b), "b"), _chk(_d(g), "g")
    bs = a.shape[0]
    da = torch.empty_like(a)
    _lib.check(lib.shdr_diff_loss_bwd_f32(_ptr(a), _ptr(b), _ptr(g), _ptr(da), bs, a.numel() // bs, mode, 0, _stream()),
               "shdr_diff_loss_bwd_f32")
    return da


def tv_loss(y):
    """batch-global TV loss (joint_training.py:175-179): tensor [1]"""
    if _needs_grad(y):
        return AUTOGRAD.tv_loss(y)
    lib = _lib.load()
    y = _chk(_d(y), "y")
    n, h, w, c = y.shape
    out = torch.empty(1, device=y.device, dtype=torch.float32)
    if DETERMINISTIC:
        ws, nws = _det_ws(_lib.DET_TV_LOSS, y.device, n=y.numel())
        _lib.check(lib.shdr_tv_loss_det_f32(_ptr(y), _ptr(out), _ptr(ws), nws, n, h, w, c, _stream()), "shdr_tv_loss_det_f32")
        return out
    _lib.check(lib.shdr_tv_loss_f32(_ptr(y), _ptr(out), n, h, w, c, _stream()), "shdr_tv_loss_f32")
    return out


def tv_loss_bwd(y, g):
    lib = _lib.load()
    y, g = _chk(_d(y), "y"), _chk(_d(g), "g")
    n, h, w, c = y.shape
    dy = torch.empty_like(y)
    _lib.check(lib.shdr_tv_loss_bwd_f32(_ptr(y), _ptr(g), _ptr(dy), n, h, w, c, 0, _stream()), "shdr_tv_loss_bwd_f32")
    return dy


def logc_bwd(dy, x):
    lib = _lib.load()
    dy, x = _chk(_d(dy), "dy"), _chk(_d(x), "x")
    dx = torch.empty_like(x)
    _lib.check(lib.shdr_logc_bwd_f32(_ptr(dy), _ptr(x), _ptr(dx), x.numel(), _stream()), "shdr_logc_bwd_f32")
    return dx


def alpha_mask(x, thr=0.12):
    """alpha [b,h,w,1] = clamp((max_c x - 1 + thr)/thr, 0, 1) (joint_training.py:141-145); no gradient."""
    lib = _lib.load()
    x, npix = _pix3(x, "x")
    alpha = torch.empty(tuple(x.shape[:-1]) + (1,), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_alpha_mask_f32(_ptr(x), _ptr(alpha), npix, float(thr), _stream()), "shdr_alpha_mask_f32")
    return alpha


def alpha_blend_bwd(dA, alpha):
    lib = _lib.load()
    dA, npix = _pix3(dA, "dA")
    alpha = _chk(_d(alpha), "alpha")
    dhal = torch.empty_like(dA)
    _lib.check(lib.shdr_alpha_blend_bwd_f32(_ptr(dA), _ptr(alpha), _ptr(dhal), npix, _stream()), "shdr_alpha_blend_bwd_f32")
    return dhal


def blend_const(base, alpha, hal_bgr, thr=0.12):
    """A = base + alpha * reverse3(hal) with base and alpha constants (joint_training.py:163-165)."""
    if _needs_grad(hal_bgr):
        return AUTOGRAD.blend_const(base, alpha, hal_bgr, thr)
    return alpha_blend(base, hal_bgr, thr)


def vgg_preprocess_bwd(dy):
    lib = _lib.load()
    if _is_h(dy):
        dy = _chkh(_d(dy), "dy")
        dx = torch.empty(tuple(dy.shape[:-1]) + (3,), device=dy.device, dtype=torch.float32)
        _lib.check(lib.shdr_unpack3_f16(_ptr(dy), _ptr(dx), None, None, None, 1, dy.shape[-1], dy.numel() // dy.shape[-1], 1, _stream()),
                   "shdr_unpack3_f16")
        return dx
    dy = _chk(_d(dy), "dy")
    ic = dy.shape[-1]
    npix = dy.numel() // ic
    dx = torch.empty(tuple(dy.shape[:-1]) + (3,), device=dy.device, dtype=torch.float32)
    _lib.check(lib.shdr_vgg_preprocess_bwd_f32(_ptr(dy), _ptr(dx), npix, ic, _stream()), "shdr_vgg_preprocess_bwd_f32")
    return dx


def adam_step(p, g, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=1.0):
    """in-place Keras Adam update of the flat parameter buffer `p`"""
    lib = _lib.load()
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(_d(t), nm)
    _lib.check(lib.shdr_adam_f32(_ptr(_d(p)), _ptr(_d(g)), _ptr(m), _ptr(v), p.numel(), float(lr_t), float(beta1), float(beta2),
                                 float(eps), float(grad_scale), _stream()), "shdr_adam_f32")
    _mutated(p, m, v)


def _mutated(*tensors):
    """The C ABI writes through raw pointers, so torch does not see an in-place update: bump the version counter (shared by a
    buffer and all its views) of every tensor a kernel has modified -- the per-version caches of the layers (zero-padded /
    x2-scaled filters, folded BatchNorm constants) key on it, and a stale cache would serve pre-update weights to an inference
    call that follows a training step."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)


def lin_frontend_bwd(img, dF):
    lib = _lib.load()
    h16 = _is_h(dF)
    img, dF = _chk(_d(img), "img"), (_chkh(_d(dF), "dF") if h16 else _chk(_d(dF), "dF"))
    n, h, w, _ = img.shape
    dimg = torch.empty_like(img)
    if h16:
        _no_det_h("lin_frontend_bwd")
    fn = "shdr_lin_frontend_bwd_f16" if h16 else ("shdr_lin_frontend_bwd_det_f32" if DETERMINISTIC else "shdr_lin_frontend_bwd_f32")
    _lib.check(getattr(lib, fn)(_ptr(img), _ptr(dF), _ptr(dimg), n, h, w, dF.shape[3], _stream()), fn)
    return dimg


def alpha_blend_full_bwd(b_pred, hal_bgr, dA, thr):
    lib = _lib.load()
    b_pred, npix = _pix3(b_pred, "b_pred")
    hal_bgr, dA = _chk(_d(hal_bgr), "hal"), _chk(_d(dA), "dA")
    dB, dhal = torch.empty_like(b_pred), torch.empty_like(b_pred)
    _lib.check(lib.shdr_alpha_blend_full_bwd_f32(_ptr(b_pred), _ptr(hal_bgr), _ptr(dA), _ptr(dB), _ptr(dhal), npix, float(thr),
                                                 _stream()), "shdr_alpha_blend_full_bwd_f32")
    return dB, dhal


def unpack3(y, nout):
    """the first `nout` 3-channel slices of y [..., C]: (y[..., 0:3], y[..., 3:6], ...)"""
    if _needs_grad(y):
        return AUTOGRAD.unpack3(y, nout)
    lib = _lib.load()
    h16 = _is_h(y)
    y = _chkh(_d(y), "y") if h16 else _chk(_d(y), "y")
    c = y.shape[-1]
    npix = y.numel() // c
    outs = [torch.empty(tuple(y.shape[:-1]) + (3,), device=y.device, dtype=torch.float32) for _ in range(nout)]
    p = [_ptr(o) for o in outs] + [None] * (4 - nout)
    if h16:
        _lib.check(lib.shdr_unpack3_f16(_ptr(y), p[0], p[1], p[2], p[3], nout, c, npix, 0, _stream()), "shdr_unpack3_f16")
        return tuple(outs)
    _lib.check(lib.shdr_unpack3_f32(_ptr(y), p[0], p[1], p[2], p[3], nout, c, npix, _stream()), "shdr_unpack3_f32")
    return tuple(outs)


def sample_dot(a, b=None):
    lib = _lib.load()
    a = _chk(_d(a), "a")
    bs = a.shape[0]
    out = torch.empty(bs, device=a.device, dtype=torch.float32)
    if DETERMINISTIC:
        ws, nws = _det_ws(_lib.DET_SAMPLE_DOT, a.device, n=a.numel() // bs, c=bs)
        _lib.check(lib.shdr_sample_dot_det_f32(_ptr(a), _ptr(None if b is None else _chk(_d(b), "b")), _ptr(out), _ptr(ws), nws, bs,
                                               a.numel() // bs, _stream()), "shdr_sample_dot_det_f32")
        return out
    _lib.check(lib.shdr_sample_dot_f32(_ptr(a), _ptr(None if b is None else _chk(_d(b), "b")), _ptr(out), bs, a.numel() // bs, _stream()),
               "shdr_sample_dot_f32")
    return out


def mean_norm(r, eps=1e-6, target=0.5):
    """r / (eps + mean over (1,2,3) of r) * target   (finetune_real_dataset.py:170)"""
    if _needs_grad(r):
        return AUTOGRAD.mean_norm(r, eps, target)
    return mean_norm_fwd(r, sample_dot(r), eps, target)


def mean_norm_fwd(r, ssum, eps, target):
    lib = _lib.load()
    r = _chk(_d(r), "r")
    bs = r.shape[0]
    out = torch.empty_like(r)
    _lib.check(lib.shdr_mean_norm_fwd_f32(_ptr(r), _ptr(ssum), _ptr(out), bs, r.numel() // bs, float(eps), float(target), _stream()),
               "shdr_mean_norm_fwd_f32")
    return out


def mean_norm_bwd(g, ssum, gdot, eps, target):
    lib = _lib.load()
    g = _chk(_d(g), "g")
    bs = g.shape[0]
    dr = torch.empty_like(g)
    _lib.check(lib.shdr_mean_norm_bwd_f32(_ptr(g), _ptr(ssum), _ptr(gdot), _ptr(dr), bs, g.numel() // bs, float(eps), float(target),
                                          _stream()), "shdr_mean_norm_bwd_f32")
    return dr


# ---------------------------------------------------------------------------
# native-fp16 path of BASELINE configs[4] (csrc/conv_f16.hip, wgrad_f16.hip, elem_f16.hip)
# ---------------------------------------------------------------------------
def to_half(x):
    lib = _lib.load()
    x = _chk(_d(x), "x")
    y = torch.empty(x.shape, device=x.device, dtype=HALF)
    _lib.check(lib.shdr_cast_f32_to_f16(_ptr(x), _ptr(y), x.numel(), _stream()), "shdr_cast_f32_to_f16")
    return y


def to_float(x):
    lib = _lib.load()
    x = _chk(_d(x), "x", HALF)
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_cast_f16_to_f32(_ptr(x), _ptr(y), x.numel(), _stream()), "shdr_cast_f16_to_f32")
    return y


def pad_channels_h(x, channels):
    """fp32 [..., c] -> fp16 [..., channels] zero-padded (the gradient of a 3-channel head onto an 8-channel group)"""
    lib = _lib.load()
    x = _chk(_d(x), "x")
    c = x.shape[-1]
    y = torch.empty(tuple(x.shape[:-1]) + (channels,), device=x.device, dtype=HALF)
    _lib.check(lib.shdr_pad_channels_f32_to_f16(_ptr(x), _ptr(y), x.numel() // c, c, channels, _stream()), "shdr_pad_channels_f32_to_f16")
    return y


def pack_filter_h(w, c1, c2=0, x2_scale=1.0):
    """fp32 HWIO filter -> the packed fp16 filter of conv2d_h ([k-chunk][Cout][32]; x2_scale folded into the x2 rows); kept ON
    the filter tensor per version for persistent variables, like the packed Winograd filters"""
    key = None
    if _is_persistent(w):
        key = (c1, c2, float(x2_scale))
        cached = _filter_cache_get(w, "_shdr_packed_h", key)
        if cached is not None:
            return cached
    lib = _lib.load()
    wd = _chk(_d(w), "w")
    kh, kw, cin, cout = wd.shape
    if cin != c1 + c2:
        raise ValueError("pack_filter_h: filter has %d input channels, sources have %d+%d" % (cin, c1, c2))
    n = int(lib.shdr_conv2d_packed_filter_elems_f16(kh, kw, c1, c2, cout))
    wp = torch.empty(n, device=wd.device, dtype=HALF)
    _lib.check(lib.shdr_conv2d_pack_filter_f16(_ptr(wd), _ptr(wp), kh, kw, c1, c2, cout, float(x2_scale), _stream()),
               "shdr_conv2d_pack_filter_f16")
    if key is not None:
        _filter_cache_put(w, "_shdr_packed_h", key, wp)
    return wp


def _conv_desc_h(x_shape, c2, khw, cout_gemm, stride, cout_valid, pad=None, out_hw=None):
    n, h, wd, c1 = x_shape
    kh, kw = khw
    ho, pt = same_pad(h, kh, stride)
    wo, pl = same_pad(wd, kw, stride)
    if pad is not None:
        pt, pl = pad
    if out_hw is not None:
        ho, wo = out_hw
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.C1, d.C2 = n, h, wd, c1, c2
    d.Cout, d.KH, d.KW, d.stride = cout_gemm, kh, kw, stride
    d.cout_valid = cout_valid or cout_gemm
    d.pad_t, d.pad_l, d.Ho, d.Wo = pt, pl, ho, wo
    d.x2_scale = 1.0
    return d


FUSED_F16_CALLS = [0]           # convolutions run through shdr_conv2d_fwd_fused_f16 (diagnostic / tests: the fp16 inference path ran)


def conv2d_h(x, wp, bias, khw, cout_gemm, stride=1, x2=None, act1=ACT_NONE, cout_valid=None, pad=None, out_hw=None, scale=None,
             shift=None, residual=None, act2=ACT_NONE):
    """y = act1(conv(concat[x, x2], wp) + bias) on fp16 feature maps, `wp` from pack_filter_h.  The output is fp16
    [N,Ho,Wo,cout_gemm], or fp32 [N,Ho,Wo,cout_valid] for a narrow head (cout_valid < cout_gemm: image-like tensors stay fp32).
    Inference epilogue (no gradient): y = act2(act1(...) * scale + shift + residual), scale / shift fp32 per output channel,
    residual fp32 or fp16 [N,Ho,Wo,>= stored channels] -- one kernel (shdr_conv2d_fwd_fused_f16)."""
    lib = _lib.load()
    x = _chkh(_d(x), "x")
    c2 = 0
    if x2 is not None:
        x2 = _chkh(_d(x2), "x2")
        if x2.shape[:3] != x.shape[:3]:
            raise ValueError("conv2d_h: x2 spatial shape %s != x %s" % (tuple(x2.shape), tuple(x.shape)))
        c2 = x2.shape[3]
    head = cout_valid is not None and cout_valid < cout_gemm
    d = _conv_desc_h(x.shape, c2, khw, cout_gemm, stride, cout_valid if head else None, pad, out_hw)
    d.act1 = act1
    if bias is not None and _chk(_d(bias), "bias").numel() < (cout_valid if head else cout_gemm):
        raise ValueError("conv2d_h: bias too short")
    y = torch.empty((x.shape[0], d.Ho, d.Wo, cout_valid if head else cout_gemm), device=x.device, dtype=torch.float32 if head else HALF)
    if scale is None and shift is None and residual is None and act2 == ACT_NONE:
        _lib.check(lib.shdr_conv2d_fwd_f16(ctypes.byref(d), _ptr(x), _ptr(x2), _ptr(wp), _ptr(_d(bias)), _ptr(y), int(head), _stream()),
                   "shdr_conv2d_fwd_f16")
        return y
    nch = y.shape[3]
    for name, v in (("scale", scale), ("shift", shift)):
        if v is not None and _chk(_d(v), name).numel() < nch:
            raise ValueError("conv2d_h: %s too short (%d < %d channels)" % (name, v.numel(), nch))
    res = None
    if residual is not None:
        res = _chk(_d(residual), "residual", HALF if _is_h(residual) else torch.float32)
        if tuple(res.shape[:3]) != (x.shape[0], d.Ho, d.Wo) or res.shape[3] < nch:
            raise ValueError("conv2d_h: residual shape %s incompatible with output %s" % (tuple(res.shape), tuple(y.shape)))
        d.res_cstride = res.shape[3]
    d.act2 = act2
    _lib.check(lib.shdr_conv2d_fwd_fused_f16(ctypes.byref(d), _ptr(x), _ptr(x2), _ptr(wp), _ptr(_d(bias)), _ptr(_d(scale)),
                                             _ptr(_d(shift)), _ptr(res), int(res is not None and res.dtype == torch.float32), _ptr(y),
                                             int(head), _stream()), "shdr_conv2d_fwd_fused_f16")
    FUSED_F16_CALLS[0] += 1
    return y


def conv2d_wgrad_h(x, x2, dz, w_shape, stride=1, x2_scale=1.0, cout_valid=None, out=None):
    """dW [kh,kw,C1+C2,Cout] (fp32) of conv(concat[x, x2_scale*x2], W) from fp16 x / x2 / dz; columns >= cout_valid stay zero.
    `out`: gradient buffer of that shape to accumulate into."""
    _no_det_h("conv2d_wgrad_h")
    lib = _lib.load()
    kh, kw, cin, cout = w_shape
    x, dz = _chkh(_d(x), "x"), _chkh(_d(dz), "dz")
    c1 = x.shape[3]
    c2 = 0 if x2 is None else x2.shape[3]
    if cin != c1 + c2:
        raise ValueError("conv2d_wgrad_h: filter %s does not match the sources (%d+%d channels)" % (tuple(w_shape), c1, c2))
    d = _conv_desc_h(x.shape, c2, (kh, kw), cout, stride, cout_valid)
    d.x2_scale = float(x2_scale)
    if tuple(dz.shape[:3]) != (x.shape[0], d.Ho, d.Wo):
        raise ValueError("conv2d_wgrad_h: dz spatial shape mismatch")
    if out is not None and (tuple(out.shape) != tuple(w_shape) or not out.is_contiguous() or out.dtype != torch.float32):
        raise ValueError("conv2d_wgrad_h: out must be a contiguous float32 tensor of shape %s" % (tuple(w_shape),))
    dw = out if out is not None else torch.zeros(tuple(w_shape), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_conv2d_wgrad_f16(ctypes.byref(d), _ptr(x), 0, _ptr(dz), dz.shape[3], c1, c2, _ptr(dw), _stream()),
               "shdr_conv2d_wgrad_f16")
    if x2 is not None:
        _lib.check(lib.shdr_conv2d_wgrad_f16(ctypes.byref(d), _ptr(_chkh(_d(x2), "x2")), 1, _ptr(dz), dz.shape[3], c1, c2, _ptr(dw),
                                             _stream()), "shdr_conv2d_wgrad_f16")
    return dw


def act_bwd_bias_h(dy, y, act, want_db, out=None):
    """(dz, db) on fp16 tensors: dz = dy * act'(y) (dy itself when act is NONE), db = sum over pixels of dz in fp32 (or None);
    `out`: gradient buffer to accumulate db into"""
    _no_det_h("act_bwd_bias_h")
    lib = _lib.load()
    dy = _chkh(_d(dy), "dy")
    c = dy.shape[-1]
    db = (out if out is not None else torch.zeros(c, device=dy.device, dtype=torch.float32)) if want_db else None
    if act == ACT_NONE:
        if want_db:
            _lib.check(lib.shdr_act_bwd_bias_f16(_ptr(dy), None, None, _ptr(db), _ptr(_bias_ws(c, dy.device)), dy.numel() // c, c, act,
                                                 _stream()), "shdr_act_bwd_bias_f16")
        return dy, db
    y = _chkh(_d(y), "y")
    dz = torch.empty_like(dy)
    ws = _bias_ws(c, dy.device) if want_db else None
    _lib.check(lib.shdr_act_bwd_bias_f16(_ptr(dy), _ptr(y), _ptr(dz), _ptr(db), _ptr(ws), dy.numel() // c, c, act, _stream()),
               "shdr_act_bwd_bias_f16")
    return dz, db


# ---------------------------------------------------------------------------
# Winograd F(2x2,3x3)
# ---------------------------------------------------------------------------
def winograd_filter(w):
    """U [16, Cin, Cout] = G g G^T of a 3x3 HWIO filter"""
    lib = _lib.load()
    w = _chk(_d(w), "w")
    kh, kw, cin, cout = w.shape
    if (kh, kw) != (3, 3):
        raise ValueError("winograd_filter: 3x3 filters only")
    u = torch.empty((16, cin, cout), device=w.device, dtype=torch.float32)
    _lib.check(lib.shdr_winograd_filter_f32(_ptr(w), _ptr(u), cin, cout, _stream()), "shdr_winograd_filter_f32")
    return u


def winograd_filter_packed(w):
    """U = G g G^T of a 3x3 HWIO filter in the operand order of the fused kernel: a [16, Cin, Cout]-sized tensor whose
    MEMORY is [Cout/64][8 waves][Cin/8][4][64 lanes][4] (see winograd_filter_packed_kernel)"""
    lib = _lib.load()
    w = _chk(_d(w), "w")
    kh, kw, cin, cout = w.shape
    if (kh, kw) != (3, 3) or cin % 8 or cout % 64:
        raise ValueError("winograd_filter_packed: 3x3 filters with Cin %% 8 == 0 and Cout %% 64 == 0 only")
    u = torch.empty((16, cin, cout), device=w.device, dtype=torch.float32)
    _lib.check(lib.shdr_winograd_filter_packed_f32(_ptr(w), _ptr(u), cin, cout, _stream()), "shdr_winograd_filter_packed_f32")
    return u


def conv2d_winograd_fused(x, u, bias=None, act1=ACT_NONE, scale=None, shift=None, act2=ACT_NONE, x2=None, pool=False):
    """3x3 / stride 1 / SAME convolution through the ONE-kernel Winograd F(2x2,3x3) (csrc/winograd_fused.hip);
    `u` from winograd_filter_packed().  `x2`: second source of a channel concatenation [x, x2] (same channel count).
    `pool=True` returns (y, MaxPool2D(2)(y)), the pooled tensor written by the same epilogue (H, W even); `pool="only"`
    returns the pooled tensor alone and y is never stored."""
    lib = _lib.load()
    x, u = _chk(_d(x), "x"), _chk(_d(u), "u")
    n, h, w, c = x.shape
    c2 = 0
    if x2 is not None:
        x2 = _chk(_d(x2), "x2")
        if tuple(x2.shape) != tuple(x.shape):
            raise ValueError("conv2d_winograd_fused: x2 %s must have the shape of x %s" % (tuple(x2.shape), tuple(x.shape)))
        c2 = c
    cout = u.shape[2]
    if u.shape[0] != 16 or u.shape[1] != c + c2 or c % 8 or cout % 64:
        raise ValueError("conv2d_winograd_fused: need u [16, Cin, Cout] with Cin %% 8 == 0 and Cout %% 64 == 0")
    y = None if pool == "only" else torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    yp = None
    if pool:
        if h % 2 or w % 2:
            raise ValueError("conv2d_winograd_fused: pool=True needs even H, W")
        yp = torch.empty((n, h // 2, w // 2, cout), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_conv2d_winograd_fused2_f32(_ptr(x), _ptr(x2), _ptr(u), _ptr(_d(bias)), _ptr(_d(scale)), _ptr(_d(shift)),
                                                   _ptr(y), _ptr(yp), n, h, w, c, c2, cout, act1, act2, _stream()),
               "shdr_conv2d_winograd_fused2_f32")
    return yp if pool == "only" else ((y, yp) if pool else y)


def _packed_filter(w):
    """winograd_filter_packed(w), kept ON the filter tensor per version for persistent variables (requires_grad leaves: the
    layers' kernels): an inference step then packs nothing (33 launches per step).  Temporaries (transposed dgrad filters)
    are packed per call.  Every kernel that rewrites a variable through a raw pointer bumps its version (_mutated, KerasAdam)."""
    if not _is_persistent(w):                      # _shdr_const: frozen weights (VGG16)
        return winograd_filter_packed(w)
    cached = _filter_cache_get(w, "_shdr_wino", "u")
    if cached is not None:
        return cached
    return _filter_cache_put(w, "_shdr_wino", "u", winograd_filter_packed(w))


def conv2d_maxpool2(x, w, bias=None, act1=ACT_NONE, keep_y=True, proj=None):
    """(y, MaxPool2D(2)(y)) with y = act1(conv(x, w) + bias): ONE launch where the planned kernel is the fused Winograd kernel
    (its epilogue writes the pooled tensor too), conv + pooling launch otherwise -- decided below the C ABI.
    keep_y=False returns the pooled tensor only.
    proj [3, Cout]: (sum_c proj[j, c] y[..., c], pooled) -- y itself is not written -- or None when the layer's planned kernel
    cannot form the projection."""
    fused = not _is_h(x) and not _needs_grad(x, w, bias) and PRECISION in ("fp32", "fp16") and WINOGRAD and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0
    if proj is not None:
        if not fused or PRECISION != "fp32":
            return None
        return _conv2d_raw(x, w, bias, 1, None, 1.0, act1, None, None, None, ACT_NONE, ALGO_AUTO, None, None, None, None, 0, True, proj=proj)
    if fused:
        return _conv2d_raw(x, w, bias, 1, None, 1.0, act1, None, None, None, ACT_NONE, ALGO_AUTO, None, None, None, None, 0,
                           True if keep_y else "only")
    y = conv2d(x, w, bias, act1=act1)
    if not keep_y:
        return maxpool2(y)
    ya, yb = fork(y)                   # the skip connection and the pooling both consume y
    return ya, maxpool2(yb)


def conv2d_avgpool2(x, w, bias=None, act1=ACT_NONE, x2=None):
    """(y, AveragePooling2D(2)(y)) with y = act1(conv(concat[x, x2], w) + bias): the encoder levels of the two U-Nets
    (dequantization_net.py:9-13 pools each level's output for the next one and keeps it as the skip connection).  Without a tape
    the pooled tensor comes out of the conv kernel's own epilogue on the split-operand plans -- decided below the C ABI."""
    if not _is_h(x) and not _needs_grad(x, w, bias, x2) and PRECISION in ("fp32", "fp16") and WINOGRAD and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0:
        return _conv2d_raw(x, w, bias, 1, x2, 1.0, act1, None, None, None, ACT_NONE, ALGO_AUTO, None, None, None, None, 0, "avg")
    y = conv2d(x, w, bias, x2=x2, act1=act1)
    ya, yb = fork(y)                   # the skip connection and the pooling both consume y
    return ya, avgpool2(yb)


def conv2d_winograd(x, u, bias=None, act1=ACT_NONE, scale=None, shift=None, act2=ACT_NONE):
    """3x3 / stride 1 / SAME convolution through Winograd F(2x2,3x3); `u` from winograd_filter()."""
    lib = _lib.load()
    x, u = _chk(_d(x), "x"), _chk(_d(u), "u")
    n, h, w, c = x.shape
    cout = u.shape[2]
    if u.shape[0] != 16 or u.shape[1] != c or c % 32 or cout % 16:
        raise ValueError("conv2d_winograd: need u [16, Cin, Cout] with Cin %% 32 == 0 and Cout %% 16 == 0")
    rows = int(lib.shdr_winograd_tiles(n, h, w))
    v = torch.empty((16, rows // 16, 16, c), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_winograd_input_f32(_ptr(x), _ptr(v), n, h, w, c, _stream()), "shdr_winograd_input_f32")
    # 16 GEMMs [rows, Cin] @ [Cin, Cout] as one "16-image" 1x1 conv; image xi uses filter plane u[xi]
    m = conv2d(v, u[0].view(1, 1, c, cout), w_batch_stride=c * cout)
    y = torch.empty((n, h, w, cout), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_winograd_output_f32(_ptr(m), _ptr(y), _ptr(_d(bias)), _ptr(_d(scale)), _ptr(_d(shift)), n, h, w, cout,
                                            act1, act2, _stream()), "shdr_winograd_output_f32")
    return y


# ---------------------------------------------------------------------------
# image plumbing of the inference tool (test_real_refinement.py:119-155), see csrc/imageio.hip
# ---------------------------------------------------------------------------
def u8_to_unit(img_u8, reverse_channels=False):
    """uint8 [..., 3] on the device -> float32 in [0,1]; optionally reversing the channel order (np.flip(img, -1))"""
    lib = _lib.load()
    if not (isinstance(img_u8, torch.Tensor) and img_u8.is_cuda and img_u8.dtype == torch.uint8 and img_u8.is_contiguous()
            and img_u8.shape[-1] == 3):
        raise TypeError("u8_to_unit: expected a contiguous uint8 device tensor [..., 3]")
    y = torch.empty(img_u8.shape, device=img_u8.device, dtype=torch.float32)
    _lib.check(lib.shdr_u8_to_unit_f32(_ptr(img_u8), _ptr(y), img_u8.numel() // 3, int(reverse_channels), _stream()),
               "shdr_u8_to_unit_f32")
    return set_bound(y, 1.0)


def resize_cubic(x, out_hw):
    """cv2.resize(x, (Wo, Ho), interpolation=cv2.INTER_CUBIC) on an NHWC float tensor"""
    lib = _lib.load()
    x = _chk(_d(x), "x")
    n, h, w, c = x.shape
    ho, wo = int(out_hw[0]), int(out_hw[1])
    y = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_resize_cubic_f32(_ptr(x), _ptr(y), n, h, w, c, ho, wo, _stream()), "shdr_resize_cubic_f32")
    return y


def pad_symmetric(x, pad):
    """np.pad(x, ((0,0),(pad,pad),(pad,pad),(0,0)), 'symmetric')"""
    lib = _lib.load()
    x = _chk(_d(x), "x")
    n, h, w, c = x.shape
    y = torch.empty((n, h + 2 * pad, w + 2 * pad, c), device=x.device, dtype=torch.float32)
    _lib.check(lib.shdr_pad_symmetric_f32(_ptr(x), _ptr(y), n, h, w, c, int(pad), _stream()), "shdr_pad_symmetric_f32")
    return y


def rgbe_encode(x, reverse_channels=False):
    """float [..., 3] -> Radiance RGBE bytes uint8 [..., 4]"""
    lib = _lib.load()
    x, npix = _pix3(x, "x")
    y = torch.empty(tuple(x.shape[:-1]) + (4,), device=x.device, dtype=torch.uint8)
    _lib.check(lib.shdr_rgbe_encode_f32(_ptr(x), _ptr(y), npix, int(reverse_channels), _stream()), "shdr_rgbe_encode_f32")
    return y


def _rle_batch(rgbe, what):
    """(flat uint8 pixels, host shape table int32 [n, 2]) of `rgbe`: one [H, W, 4] or [N, H, W, 4] tensor (used as it is, no copy) or a
    list of [H, W, 4] tensors of different sizes (packed back to back on the device)"""
    def chk(t):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() in (3, 4) and t.shape[-1] == 4):
            raise TypeError("%s: expected uint8 RGBE device tensors [H, W, 4] or [N, H, W, 4] (see rgbe_encode)" % what)
        if t.numel() == 0:
            raise ValueError("%s: an image has no pixels: %s" % (what, tuple(t.shape)))
        return t.contiguous()
    if isinstance(rgbe, (list, tuple)):
        if not rgbe:
            raise ValueError("%s: no images" % what)
        imgs = [chk(t) for t in rgbe]
        if any(t.dim() != 3 for t in imgs):
            raise TypeError("%s: a list holds single images [H, W, 4]" % what)
        shapes = np.array([t.shape[:2] for t in imgs], dtype=np.int32)
        flat = imgs[0].reshape(-1) if len(imgs) == 1 else torch.cat([t.reshape(-1) for t in imgs])
        return flat, shapes
    t = chk(rgbe)
    n = 1 if t.dim() == 3 else t.shape[0]
    return t.reshape(-1), np.tile(np.array(t.shape[-3:-1], dtype=np.int32), (n, 1))


def rgbe_rle_encode(rgbe, capacity=None, stage_ms=None):
    """Radiance scanline bytes of RGBE images, coded on the device (csrc/hdr_rle.hip): byte for byte what the host routine
    shdr_rgbe_rle_encode (hdr_io.rle_encode) writes.  rgbe: uint8 device tensor [H, W, 4] or [N, H, W, 4] (the layout rgbe_encode
    returns: no copy), or a list of [H, W, 4] tensors of different sizes.  Returns (bytes uint8 [capacity], offsets int64 [N + 1]) on
    the device: image i is bytes[offsets[i]:offsets[i + 1]].  Stream-ordered, no host wait.  capacity: size of the output buffer
    (default and minimum: the host routine's bound); stage_ms: a list that receives the four launches' device times (measurement: the
    call then waits)."""
    lib = _lib.load()
    flat, shapes = _rle_batch(rgbe, "rgbe_rle_encode")
    n = shapes.shape[0]
    out_b, ws_b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.shdr_rgbe_rle_encode_batch_sizes(_hptr(shapes), n, ctypes.byref(out_b), ctypes.byref(ws_b)),
               "shdr_rgbe_rle_encode_batch_sizes")
    dev = flat.device
    cap = out_b.value if capacity is None else int(capacity)
    out = torch.empty(max(cap, 1), device=dev, dtype=torch.uint8)
    offsets = torch.empty(n + 1, device=dev, dtype=torch.int64)
    ws = torch.empty(ws_b.value, device=dev, dtype=torch.uint8)
    shapes_dev = torch.from_numpy(shapes).to(dev)
    args = (_ptr(flat), _hptr(shapes), _ptr(shapes_dev), n, _ptr(out), cap, _ptr(offsets), _ptr(ws), _stream())
    with _stage_times(stage_ms, 4) as ms:
        if ms is None:
            _lib.check(lib.shdr_rgbe_rle_encode_batch(*args), "shdr_rgbe_rle_encode_batch")
        else:
            _lib.check(lib.shdr_rgbe_rle_encode_batch_timed(*args, ms), "shdr_rgbe_rle_encode_batch_timed")
    return out, offsets


# SHDR_RGBE_DEC_* (include/shdr.h) -> the words of shdr_rgbe_rle_decode's messages; FALLBACK is no failure (the host routine decodes)
RGBE_DEC_OK, RGBE_DEC_TRUNCATED, RGBE_DEC_CORRUPT_RUN, RGBE_DEC_CORRUPT_LITERAL, RGBE_DEC_TRUNCATED_FLAT, RGBE_DEC_FALLBACK = range(6)
RGBE_DEC_REASONS = {
    RGBE_DEC_TRUNCATED: "truncated data in scanline %d",
    RGBE_DEC_CORRUPT_RUN: "corrupt run in scanline %d",
    RGBE_DEC_CORRUPT_LITERAL: "corrupt literal in scanline %d",
    RGBE_DEC_TRUNCATED_FLAT: "truncated data in flat scanline %d",
}


def rgbe_dec_message(status, line):
    """the text shdr_rgbe_rle_decode leaves in shdr_last_error for a file refused with (status, line)"""
    if status not in RGBE_DEC_REASONS:
        raise ValueError("rgbe_dec_message: status %r is no refusal" % (status,))
    return "rgbe_rle_decode: " + RGBE_DEC_REASONS[status] % line


def rgbe_rle_decode_host(data, w, h):
    """scanline bytes of one Radiance file -> (pixels uint8 [h, w, 4] or None, status, line, consumed): libshdr's host twin of
    shdr_rgbe_rle_decode (csrc/hdr_rle_dec.h, the rules the kernels run).  consumed: the bytes consumed, or for a refused file the
    offset at which the reader stood"""
    lib = _lib.load()
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    w, h = int(w), int(h)
    if w <= 0 or h <= 0:
        raise ValueError("rgbe_rle_decode_host: the image is %d x %d (H x W): sizes must be positive" % (h, w))
    out = np.zeros((h, w, 4), dtype=np.uint8)
    st, ln, stop = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int64(-1)
    n = lib.shdr_rgbe_rle_decode_status(_hptr(src) if src.size else None, src.size, w, h, _hptr(out), ctypes.byref(st), ctypes.byref(ln),
                                        ctypes.byref(stop))
    if st.value < 0:
        raise RuntimeError("shdr_rgbe_rle_decode_status: %s" % lib.shdr_last_error().decode())
    if st.value != RGBE_DEC_OK:
        return None, st.value, ln.value, stop.value
    return out, st.value, ln.value, n


def rgbe_rle_decode(src, src_off, shapes, stage_ms=None):
    """Radiance scanline bytes of a batch of files decoded on the device (csrc/hdr_rle_dec.hip): the pixels, refusals and consumed counts
    of the host routine shdr_rgbe_rle_decode.  src: uint8 device tensor, the files' scanline data back to back; src_off: int64 [n + 1]
    (host: array or list), file i is src[src_off[i]:src_off[i + 1]]; shapes: int32 [n, 2] = (H, W) (host).  Returns device tensors
    (out uint8, out_off int64 [n + 1], status int32 [n], line int32 [n], consumed int64 [n]): file i is
    out[out_off[i]:out_off[i + 1]].view(H, W, 4) when status[i] is 0; RGBE_DEC_FALLBACK: not decoded here (more line markers than
    2 H + 64), its slot is untouched; any other status: refused as the host routine refuses it, in scanline line[i], the reader standing
    at consumed[i].  Stream-ordered, no host wait.  stage_ms: a list that receives the four stages' device times (measurement: the call
    then waits)."""
    lib = _lib.load()
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.dim() == 1):
        raise TypeError("rgbe_rle_decode: src must be a flat uint8 device tensor")
    src = src.contiguous()
    shapes = np.ascontiguousarray(shapes, dtype=np.int32).reshape(-1, 2)
    s_host = np.ascontiguousarray(src_off, dtype=np.int64).reshape(-1)
    n = shapes.shape[0]
    if s_host.size != n + 1:
        raise ValueError("rgbe_rle_decode: %d shapes need %d offsets, got %d" % (n, n + 1, s_host.size))
    out_b, ws_b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.shdr_rgbe_rle_decode_batch_sizes(_hptr(shapes), _hptr(s_host), n, ctypes.byref(out_b), ctypes.byref(ws_b)),
               "shdr_rgbe_rle_decode_batch_sizes")
    dev = src.device
    out = torch.empty(max(out_b.value, 4), device=dev, dtype=torch.uint8)
    ws = torch.empty(max(ws_b.value, 16), device=dev, dtype=torch.uint8)
    out_off = torch.empty(n + 1, device=dev, dtype=torch.int64)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    line = torch.empty(n, device=dev, dtype=torch.int32)
    consumed = torch.empty(n, device=dev, dtype=torch.int64)
    s_dev = torch.from_numpy(s_host).to(dev)
    shapes_dev = torch.from_numpy(shapes).to(dev)
    with _stage_times(stage_ms, 4) as ms:
        _lib.check(lib.shdr_rgbe_rle_decode_batch(_ptr(src) if src.numel() else None, src.numel(), _hptr(s_host), _ptr(s_dev), _hptr(shapes),
                                                  _ptr(shapes_dev), n, _ptr(out), out_b.value, _ptr(out_off), _ptr(ws), ws_b.value,
                                                  _ptr(status), _ptr(line), _ptr(consumed), _stream(), ms), "shdr_rgbe_rle_decode_batch")
    return out, out_off, status, line, consumed


# ---------------------------------------------------------------------------
# camera-pipeline simulator (joint_training.py:26-69), see csrc/camera.hip
# ---------------------------------------------------------------------------
def camera_expose(hdr, t, seed):
    """(hdr_t, clipped_hdr_t) of joint_training.py:30-43: exposure, shot + read noise, relu, clip to [0,1]"""
    lib = _lib.load()
    hdr, npix = _pix3(hdr, "hdr")
    t = _chk(_d(t), "t").reshape(-1)
    n, h, w, _ = hdr.shape
    if t.numel() != n:
        raise ValueError("camera_expose: t must have one exposure per sample")
    hdr_t, clipped = torch.empty_like(hdr), torch.empty_like(hdr)
    _lib.check(lib.shdr_camera_expose_f32(_ptr(hdr), _ptr(t), _ptr(hdr_t), _ptr(clipped), n, h, w, int(seed) & (2 ** 64 - 1),
                                          _stream()), "shdr_camera_expose_f32")
    return hdr_t, clipped


def jpeg_round_trip(ldr, quality):
    """(jpeg_img_float, loss_mask [b,1,1,1]) of joint_training.py:46-63; `quality`: one int per sample"""
    lib = _lib.load()
    ldr, npix = _pix3(ldr, "ldr")
    n, h, w, _ = ldr.shape
    q = torch.as_tensor(list(quality), dtype=torch.int32).to(ldr.device) if not isinstance(quality, torch.Tensor) else quality
    if q.dtype != torch.int32 or q.numel() != n or not q.is_cuda:
        raise ValueError("jpeg_round_trip: quality must be %d int32 values" % n)
    jpeg = torch.empty_like(ldr)
    mask = torch.empty((n, 1, 1, 1), device=ldr.device, dtype=torch.float32)
    planes = torch.empty(n * h * w * 3 // 2, device=ldr.device, dtype=torch.uint8)
    counts = torch.empty(2 * n, device=ldr.device, dtype=torch.int32)
    _lib.check(lib.shdr_jpeg_round_trip_f32(_ptr(ldr), _ptr(q), _ptr(jpeg), _ptr(mask), _ptr(planes), _ptr(counts), n, h, w,
                                            _stream()), "shdr_jpeg_round_trip_f32")
    return jpeg, mask


def flip_rot90(x, flip, rot, divisor=1.0):
    """per-sample rot90(flip_left_right(x) if flip else x, k) / divisor on square NHWC images; flip / rot: int32 [N] on the device"""
    lib = _lib.load()
    x = _chk(_d(x), "x")
    n, h, w, c = x.shape
    if h != w:
        raise ValueError("flip_rot90: square images only, got %dx%d" % (h, w))
    for t, nm in ((flip, "flip"), (rot, "rot")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.numel() == n):
            raise TypeError("flip_rot90: %s must be %d int32 values on the device" % (nm, n))
    y = torch.empty_like(x)
    _lib.check(lib.shdr_flip_rot90_f32(_ptr(x), _ptr(y), _ptr(flip), _ptr(rot), n, h, c, float(divisor), _stream()),
               "shdr_flip_rot90_f32")
    return y


# ---------------------------------------------------------------------------
# training-set patch sampler (dataset.py:141-252), see csrc/dataset.hip
# ---------------------------------------------------------------------------
def hdr_load_resize(rgbe, out):
    """RGBE bytes uint8 [H0, W0, 4] on the device -> float BGR, cv2-linear resized into `out` [H, W, 3] (a view of the arena)"""
    lib = _lib.load()
    rgbe = _chk(rgbe, "rgbe", torch.uint8)
    out = _chk(out, "out")
    if rgbe.dim() != 3 or rgbe.shape[2] != 4 or out.dim() != 3 or out.shape[2] != 3:
        raise ValueError("hdr_load_resize: expected rgbe [H0, W0, 4] and out [H, W, 3]")
    h0, w0, _ = rgbe.shape
    h, w, _ = out.shape
    _lib.check(lib.shdr_hdr_load_resize_f32(_ptr(rgbe), _ptr(out), h0, w0, h, w, _stream()), "shdr_hdr_load_resize_f32")
    return out


def hdr_window_means(arena, offsets, dims):
    """np.mean of both 512 x 512 crops of every resident image: float32 [2 * n_files] (file f, parity p at 2 f + p)"""
    lib = _lib.load()
    arena = _chk(arena, "arena")
    offsets = _chk(offsets, "offsets", torch.int64)
    dims = _chk(dims, "dims", torch.int32)
    n = offsets.numel()
    if dims.numel() != 2 * n:
        raise ValueError("hdr_window_means: dims must be [n_files, 2]")
    partials = torch.empty(2 * n * 64, device=arena.device, dtype=torch.float32)
    means = torch.empty(2 * n, device=arena.device, dtype=torch.float32)
    _lib.check(lib.shdr_hdr_window_means_f32(_ptr(arena), _ptr(offsets), _ptr(dims), n, _ptr(partials), _ptr(means), _stream()),
               "shdr_hdr_window_means_f32")
    return means


def hdr_patch_sample(arena, offsets, dims, means, params, P):
    """one PatchHDRDataset.__getitem__ per row of `params` (int32 [N, >= 7] on the device: idx, S, y0, x0, k, flip0, flip1)
    -> float32 [N, P, P, 3].  The caller validates the parameters (dataset.PatchHDRDataset.render does)."""
    lib = _lib.load()
    arena = _chk(arena, "arena")
    offsets = _chk(offsets, "offsets", torch.int64)
    dims = _chk(dims, "dims", torch.int32)
    means = _chk(means, "means")
    params = _chk(params, "params", torch.int32)
    if params.dim() != 2 or params.shape[1] < 7:
        raise ValueError("hdr_patch_sample: params must be int32 [N, >= 7]")
    n = params.shape[0]
    y = torch.empty((n, P, P, 3), device=arena.device, dtype=torch.float32)
    _lib.check(lib.shdr_hdr_patch_sample_f32(_ptr(arena), _ptr(offsets), _ptr(dims), _ptr(means), _ptr(params), params.shape[1], n,
                                             offsets.numel(), int(P), _ptr(y), _stream()), "shdr_hdr_patch_sample_f32")
    return y


# ---------------------------------------------------------------------------
# OpenEXR training files (exr.py), see csrc/exr.hip
# ---------------------------------------------------------------------------
def exr_unpredict(payload, offsets, coded):
    """uint8 chunk bytes on the device (chunk c at [offsets[c], offsets[c + 1]), int64 [n + 1]) -> the scanline bytes: the
    RLE / ZIP predictor and byte interleave undone where coded[c] (uint8 [n]) is set, copied elsewhere"""
    lib = _lib.load()
    payload = _chk(payload, "payload", torch.uint8)
    offsets = _chk(offsets, "offsets", torch.int64)
    coded = _chk(coded, "coded", torch.uint8)
    n = coded.numel()
    if payload.dim() != 1 or offsets.numel() != n + 1:
        raise ValueError("exr_unpredict: expected payload [size], offsets [n_chunks + 1] and coded [n_chunks]")
    out = torch.empty_like(payload)
    _lib.check(lib.shdr_exr_unpredict_u8(_ptr(payload), _ptr(out), payload.numel(), _ptr(offsets), _ptr(coded), n, _stream()),
               "shdr_exr_unpredict_u8")
    return out


def exr_load_resize(planes, offsets, lines, row_bytes, chan_off, chan_type, h0, w0, out, clip=False):
    """planar OpenEXR scanlines on the device (of exr_unpredict) -> float32, cv2-linear resized into `out` [H, W, 3]; output
    channel i is the run at byte chan_off[i] of each scanline, of type chan_type[i] (1 HALF, 2 FLOAT); clip: np.clip(x, 0, None)
    before the resize"""
    lib = _lib.load()
    planes = _chk(planes, "planes", torch.uint8)
    offsets = _chk(offsets, "offsets", torch.int64)
    out = _chk(out, "out")
    if planes.dim() != 1 or out.dim() != 3 or out.shape[2] != 3 or len(chan_off) != 3 or len(chan_type) != 3:
        raise ValueError("exr_load_resize: expected planes [size], out [H, W, 3] and three channels")
    h, w, _ = out.shape
    off = (ctypes.c_int64 * 3)(*[int(v) for v in chan_off])
    typ = (ctypes.c_int32 * 3)(*[int(v) for v in chan_type])
    _lib.check(lib.shdr_exr_load_resize_f32(_ptr(planes), planes.numel(), _ptr(offsets), offsets.numel() - 1, int(lines),
                                            int(row_bytes), off, typ, int(h0), int(w0), _ptr(out), h, w, int(bool(clip)),
                                            _stream()), "shdr_exr_load_resize_f32")
    return out


# ---------------------------------------------------------------------------
# what the batched byte coders below (deflate, inflate, the JPEG scan) share: offset tables and stage times
# ---------------------------------------------------------------------------
def _offsets_pair(what, name, offsets, offsets_dev):
    """(host int64 array, device tensor or None) of an offset table given as a host array (+ the caller's device copy) or a tensor"""
    if isinstance(offsets, torch.Tensor):
        host = np.ascontiguousarray(offsets.detach().cpu().numpy(), dtype=np.int64)
        dev = offsets if offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() else None
    else:
        host, dev = np.ascontiguousarray(offsets, dtype=np.int64), offsets_dev
        if dev is not None and _chk(dev, name + "_dev", torch.int64).numel() != host.size:
            raise ValueError("%s: %s_dev is not a copy of %s" % (what, name, name))
    if host.ndim != 1 or host.size < 2:
        raise ValueError("%s: %s must be [n_chunks + 1]" % (what, name))
    return host, dev


class _stage_times:
    """with _stage_times(stage_ms, n) as ms: the float [n] that a library call fills with the device times of its n stages, or None
    where the caller gave no list (stage_ms is None); after the call the times replace the contents of the list"""

    def __init__(self, stage_ms, n):
        self._list, self._ms = stage_ms, (ctypes.c_float * n)() if stage_ms is not None else None

    def __enter__(self):
        return self._ms

    def __exit__(self, exc_type, *exc):
        if exc_type is None and self._ms is not None:
            self._list[:] = list(self._ms)
        return False


def _slot_batch(what, src, src_offsets, dst_offsets, src_offsets_dev, dst_offsets_dev, dst, mode, sizes):
    """inflate and piz_decode: chunk c of src fills slot c of dst.  The checks and buffers of both: src, the two offset tables with
    their device copies, dst (made if None), mode, and the per-chunk status and written.  sizes(src, s_host, d_host, n) refuses tables
    whose shapes do not fit and returns the library's (src bytes, dst bytes).  Returns (src, (s_host, s_dev), (d_host, d_dev), dst, mode,
    status, written)."""
    src = _chk(src, "src", torch.uint8)
    s_host, s_dev = _offsets_pair(what, "src_offsets", src_offsets, src_offsets_dev)
    d_host, d_dev = _offsets_pair(what, "dst_offsets", dst_offsets, dst_offsets_dev)
    n = s_host.size - 1
    src_b, dst_b = sizes(src, s_host, d_host, n)
    if src_b > src.numel():
        raise ValueError("%s: src_offsets end at %d, src holds %d bytes" % (what, src_b, src.numel()))
    dev = src.device
    if dst is None:
        dst = torch.empty(dst_b, device=dev, dtype=torch.uint8)
    else:
        dst = _chk(dst, "dst", torch.uint8)
        if dst.dim() != 1 or dst.numel() < dst_b:
            raise ValueError("%s: dst_offsets end at %d, dst holds %d bytes" % (what, dst_b, dst.numel()))
    if mode is not None:
        mode = _chk(mode, "mode", torch.uint8)
        if mode.numel() != n:
            raise ValueError("%s: mode must be uint8 [n_chunks]" % what)
    if s_dev is None:
        s_dev = torch.from_numpy(s_host).to(dev)
    if d_dev is None:
        d_dev = torch.from_numpy(d_host).to(dev)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    written = torch.empty(n, device=dev, dtype=torch.int64)
    return src, (s_host, s_dev), (d_host, d_dev), dst, mode, status, written


def _shape_tables(what, geom, chan_words, shape_dev, n, dev):
    """piz_decode and piz_encode: (geom, chan_words) on the device -- the caller's copies shape_dev, checked, or one upload of both"""
    if shape_dev is None:
        both = torch.from_numpy(np.concatenate([geom.reshape(-1), chan_words])).to(dev)
        return both[:4 * n], both[4 * n:]
    geom_dev, words_dev = _chk(shape_dev[0], "geom_dev", torch.int32), _chk(shape_dev[1], "chan_words_dev", torch.int32)
    if geom_dev.numel() != 4 * n or words_dev.numel() != chan_words.size:
        raise ValueError("%s: shape_dev is not a copy of geom and chan_words" % what)
    return geom_dev, words_dev


def _store_buffers(what, out, front, out_bytes, ws_bytes, n, dev):
    """the deflate encoders and piz_encode: (out, out_offsets, coded, workspace) of a call that stores n chunks of at most out_bytes
    behind `front` free bytes; out: the caller's buffer, checked, or None for a new one (not cleared)"""
    if out is None:
        out = torch.empty(front + out_bytes, device=dev, dtype=torch.uint8)
    else:
        out = _chk(out, "out", torch.uint8)
        if out.dim() != 1 or out.numel() < front + out_bytes:
            raise ValueError("%s: out holds %d bytes, %d are needed" % (what, out.numel(), front + out_bytes))
    return (out, torch.empty(n + 1, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.uint8),
            torch.empty(ws_bytes, device=dev, dtype=torch.uint8))


# ---------------------------------------------------------------------------
# OpenEXR output (exr.py encode_exr), see csrc/exr_write.hip and csrc/deflate.hip
# ---------------------------------------------------------------------------
DEFLATE_TILE = 1024          # SHDR_DEFLATE_TILE: symbols per tile of the device writer


def _deflate_host(fn_name, chunk):
    """deflate_huffman_host and deflate_lz_host: the stream that the library's host routine `fn_name` writes for a chunk"""
    lib = _lib.load()
    src = np.frombuffer(bytes(chunk), dtype=np.uint8)
    out = np.empty(2 * src.size + 512, dtype=np.uint8)                    # a header of 1122 or 1354 bits + 16 per byte at the very most
    n = getattr(lib, fn_name)(_hptr(src), src.size, _hptr(out), out.size)
    if n < 0:
        raise ValueError(lib.shdr_last_error().decode())
    return out[:n].tobytes()


def deflate_huffman_host(chunk):
    """Huffman-only zlib stream of a chunk of bytes (libshdr host routine; zlib.decompress reads it).  The stream is returned
    whatever its size: a chunk counts as coded only if len(stream) < len(chunk)"""
    return _deflate_host("shdr_deflate_huffman_host", chunk)


def deflate_huffman_lengths_host(chunk):
    """the 257 code lengths (literals, end-of-block) of deflate_huffman_host's stream: uint8 [257]"""
    lib = _lib.load()
    src = np.frombuffer(bytes(chunk), dtype=np.uint8)
    out = np.empty(257, dtype=np.uint8)
    rc = lib.shdr_deflate_huffman_lengths_host(_hptr(src), src.size, _hptr(out))
    if rc != 0:
        raise ValueError(lib.shdr_last_error().decode())
    return out


def _deflate_batch(what, sizes_fn_name, batch_fn_name, data, offsets, raw, pad, front, stage_ms, offsets_dev):
    """deflate_huffman and deflate_lz: the same arguments, buffers and call; the two library symbols differ"""
    lib = _lib.load()
    data = _chk(data, "data", torch.uint8)
    off_host, off_dev = _offsets_pair(what, "offsets", offsets, offsets_dev)
    if data.dim() != 1 or int(off_host[-1]) > data.numel():
        raise ValueError("%s: expected data [size] and offsets [n_chunks + 1] that end within it" % what)
    if raw is not None:
        raw = _chk(raw, "raw", torch.uint8)
        if raw.dim() != 1 or raw.numel() < int(off_host[-1]):
            raise ValueError("%s: raw must hold the chunks' bytes too" % what)
    n = off_host.size - 1
    out_b, ws_b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(getattr(lib, sizes_fn_name)(_hptr(off_host), n, int(pad), ctypes.byref(out_b), ctypes.byref(ws_b)), sizes_fn_name)
    dev = data.device
    if off_dev is None:
        off_dev = torch.from_numpy(off_host).to(dev)
    front = int(front)
    out, out_offsets, coded, ws = _store_buffers(what, None, front, out_b.value, ws_b.value, n, dev)
    with _stage_times(stage_ms, 3) as ms:
        _lib.check(getattr(lib, batch_fn_name)(_ptr(data), _ptr(raw) if raw is not None else None, _hptr(off_host), _ptr(off_dev), n, int(pad),
                                               out.data_ptr() + front, out_b.value, _ptr(out_offsets), _ptr(coded), _ptr(ws), _stream(), ms),
                   batch_fn_name)
    return out, out_offsets, coded


def deflate_huffman(data, offsets, raw=None, pad=0, front=0, stage_ms=None, offsets_dev=None):
    """Huffman-only zlib streams of a batch of chunks, coded on the device (csrc/deflate.hip): byte for byte what the host routine
    shdr_deflate_huffman_host writes.  data: uint8 device tensor; offsets: int64 [n + 1] (host array or tensor), chunk c is
    data[offsets[c]:offsets[c + 1]], at least 1 byte.  Returns (bytes, out_offsets int64 [n + 1], coded uint8 [n]) on the device:
    chunk c is stored at bytes[front + out_offsets[c] + pad : front + out_offsets[c + 1]] -- its stream where coded[c], else (the
    stream would not be strictly smaller) the chunk's bytes of `raw` (default: of `data`) as they are.  pad: bytes left free in front
    of every stored chunk; front: bytes left free in front of all of them.  Stream-ordered, no host wait.  stage_ms: a list that
    receives the three launches' device times (measurement: the call then waits); offsets_dev: the device copy of a host `offsets`,
    if the caller has one."""
    return _deflate_batch("deflate_huffman", "shdr_deflate_huffman_batch_sizes", "shdr_deflate_huffman_batch", data, offsets, raw, pad, front,
                          stage_ms, offsets_dev)


DEFLATE_LZ_TILE = 1024       # SHDR_DEFLATE_LZ_TILE: positions per tile of the device writer of deflate_lz
DEFLATE_LZ_LITERAL = 0x80000000   # SHDR_DEFLATE_LZ_LITERAL


def deflate_lz_host(chunk):
    """zlib stream with LZ77 matches of a chunk of bytes (libshdr host routine, csrc/deflate_lz.h; zlib.decompress reads it).  The
    stream is returned whatever its size: a chunk counts as coded only if len(stream) < len(chunk)"""
    return _deflate_host("shdr_deflate_lz_host", chunk)


def deflate_lz_parse_host(chunk):
    """the parse behind deflate_lz_host's stream: a list of (position, length, distance), one per token in stream order; a literal
    has length 1 and distance 0, a match 3..258 and 1..32768"""
    lib = _lib.load()
    src = np.frombuffer(bytes(chunk), dtype=np.uint8)
    tokens = np.empty(max(src.size, 1), dtype=np.uint32)
    rc = lib.shdr_deflate_lz_parse_host(_hptr(src), src.size, _hptr(tokens))
    if rc != 0:
        raise ValueError(lib.shdr_last_error().decode())
    at = np.flatnonzero(tokens)
    t = tokens[at].astype(np.int64)
    lit = (t & DEFLATE_LZ_LITERAL) != 0
    length = np.where(lit, 1, t >> 16)
    dist = np.where(lit, 0, t & 0xFFFF)
    return list(zip(at.tolist(), length.tolist(), dist.tolist()))


def deflate_lz(data, offsets, raw=None, pad=0, front=0, stage_ms=None, offsets_dev=None):
    """zlib streams with LZ77 matches of a batch of chunks, coded on the device (csrc/deflate_lz.hip): byte for byte what the host
    routine shdr_deflate_lz_host writes.  Arguments and the returned (bytes, out_offsets, coded) as deflate_huffman; the workspace
    holds 4 bytes per input byte for the parse's tokens.  stage_ms: the device times of the parse, scan and write launches."""
    return _deflate_batch("deflate_lz", "shdr_deflate_lz_batch_sizes", "shdr_deflate_lz_batch", data, offsets, raw, pad, front, stage_ms,
                          offsets_dev)


# ---------------------------------------------------------------------------
# zlib streams inflated (exr.py read_stored / upload_batch), see csrc/inflate.h and csrc/inflate.hip
# ---------------------------------------------------------------------------
INFLATE_REASONS = (                                   # SHDR_INFLATE_*: the per-chunk status of the host routine and of the kernel
    "ok", "truncated stream", "bad zlib header", "preset dictionary", "invalid block type", "invalid stored block lengths",
    "too many length or distance symbols", "invalid code lengths set", "invalid bit length repeat", "code length run overflows",
    "missing end-of-block", "invalid literal/lengths set", "invalid distances set", "invalid literal/length code",
    "invalid distance code", "invalid distance too far back", "output longer than its slot", "output shorter than its slot",
    "incorrect data check", "raw chunk size is not its slot's", "invalid mode byte")


def inflate_reason(status):
    status = int(status)
    return INFLATE_REASONS[status] if 0 <= status < len(INFLATE_REASONS) else "status %d" % status


def inflate_host(stream, capacity):
    """a zlib stream -> (bytes, status): libshdr's host decoder (csrc/inflate.h, the code the kernel runs).  capacity: the size the
    output must have; status 0 means exactly that many bytes came out and the Adler-32 holds, any other value is an index into
    INFLATE_REASONS and `bytes` is what had been written by then (never more than capacity)"""
    lib = _lib.load()
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    capacity = int(capacity)
    out = np.empty(max(capacity, 1), dtype=np.uint8)
    st = ctypes.c_int(-1)
    n = lib.shdr_inflate_host(_hptr(src) if src.size else None, src.size, _hptr(out), capacity, ctypes.byref(st))
    if n < 0:
        raise ValueError(lib.shdr_last_error().decode())
    return out[:n].tobytes(), st.value


def inflate(src, src_offsets, dst_offsets, mode=None, stage_ms=None, src_offsets_dev=None, dst_offsets_dev=None, dst=None):
    """a batch of zlib streams inflated on the device in one launch (csrc/inflate.hip): chunk c is src[src_offsets[c]:src_offsets[c + 1]]
    and is written into the slot dst[dst_offsets[c]:dst_offsets[c + 1]], which its output must fill exactly.  src: uint8 device tensor;
    the offsets: int64 [n + 1], non-decreasing (host arrays or tensors; *_dev: the device copies of host arrays, if the caller has
    them); mode: uint8 [n] on the device, 1 a zlib stream, 0 stored raw (copied if its size is the slot's), default all 1; dst: a
    uint8 device tensor of at least dst_offsets[-1] bytes to write into (default: a new one of that size, not cleared).  Returns
    (dst, written int64 [n], status int32 [n]) on the device: status 0, or an index into INFLATE_REASONS; bytes of a slot beyond
    `written` are left as they were.  Stream-ordered, no host wait.  stage_ms: a list that receives the launch's device time
    (measurement: the call then waits)."""
    lib = _lib.load()

    def sizes(src, s_host, d_host, n):
        if src.dim() != 1 or d_host.size != n + 1:
            raise ValueError("inflate: expected src [size] and two offset tables [n_chunks + 1]")
        src_b, dst_b = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(lib.shdr_inflate_batch_sizes(_hptr(s_host), _hptr(d_host), n, ctypes.byref(src_b), ctypes.byref(dst_b)),
                   "shdr_inflate_batch_sizes")
        return src_b.value, dst_b.value

    src, (s_host, s_dev), (d_host, d_dev), dst, mode, status, written = _slot_batch(
        "inflate", src, src_offsets, dst_offsets, src_offsets_dev, dst_offsets_dev, dst, mode, sizes)
    n = s_host.size - 1
    with _stage_times(stage_ms, 1) as ms:
        _lib.check(lib.shdr_inflate_batch(_ptr(src) if src.numel() else None, src.numel(), _hptr(s_host), _ptr(s_dev),
                                          _ptr(dst) if dst.numel() else None, dst.numel(), _hptr(d_host), _ptr(d_dev),
                                          _ptr(mode) if mode is not None else None, n, _ptr(status), _ptr(written), _stream(), ms),
                   "shdr_inflate_batch")
    return dst, written, status


# ---------------------------------------------------------------------------
# OpenEXR PIZ chunks decoded (exr.py piz="host" / "device"), see csrc/piz.h and csrc/piz.hip
# ---------------------------------------------------------------------------
PIZ_REASONS = (                                       # SHDR_PIZ_*: the per-chunk status of the host routine and of the kernels
    "ok", "truncated chunk", "invalid bitmap range", "invalid Huffman block length", "no data", "invalid Huffman header",
    "truncated code-length table", "code-length run overflows", "over-subscribed code lengths", "nBits beyond the data", "invalid code",
    "truncated data", "run with no previous value", "more values than the chunk holds", "fewer values than the chunk holds",
    "raw chunk size is not its slot's", "invalid mode byte")
PIZ_ROUND_STATS = 9                                   # SHDR_PIZ_ROUND_STATS
PIZ_MIN_SUB_BITS, PIZ_SUB_BITS = 128, 256             # the smallest legal and the default subsequence of the device decoder


def piz_reason(status):
    status = int(status)
    return PIZ_REASONS[status] if 0 <= status < len(PIZ_REASONS) else "status %d" % status


def piz_decode_host(chunk, width, rows, chan_words, out=None):
    """one PIZ chunk -> (bytes, status): libshdr's host decoder (csrc/piz.h, the rules the kernels run).  chan_words: 1 per HALF
    channel, 2 per FLOAT / UINT channel, in name order.  status 0: `bytes` are the 2 * width * rows * sum(chan_words) bytes of the
    chunk's planar scanlines; any other value is an index into PIZ_REASONS and `bytes` is empty.  out: a uint8 array of exactly that
    size to decode into (then returned instead of bytes, left untouched by a refused chunk)."""
    lib = _lib.load()
    src = np.frombuffer(chunk, dtype=np.uint8) if not isinstance(chunk, np.ndarray) else chunk
    words = np.ascontiguousarray(chan_words, dtype=np.int32)
    capacity = 2 * int(width) * int(rows) * int(words.sum())
    buf = np.empty(max(capacity, 1), dtype=np.uint8) if out is None else out
    st = ctypes.c_int(-1)
    n = lib.shdr_piz_decode_host(src.ctypes.data if src.size else None, src.size, int(width), int(rows), _hptr(words), words.size,
                                 buf.ctypes.data, capacity if out is None else buf.size, ctypes.byref(st))
    if n < 0:
        raise ValueError(lib.shdr_last_error().decode())
    return (buf[:n].tobytes() if out is None else buf), st.value


def piz_decode(src, src_offsets, dst_offsets, geom, chan_words, mode=None, sub_bits=None, stage_ms=None, src_offsets_dev=None,
               dst_offsets_dev=None, dst=None, shape_dev=None, rounds=False):
    """a batch of PIZ chunks decoded on the device (csrc/piz.hip: Huffman decode by self-synchronising subsequences, then the inverse
    wavelet and the LUT): chunk c is src[src_offsets[c]:src_offsets[c + 1]] and fills the slot dst[dst_offsets[c]:dst_offsets[c + 1]]
    with its planar scanlines.  geom: int32 [n, 4] host array (width, rows, first entry and number of entries in chan_words);
    chan_words: int32 host array, 1 per HALF channel and 2 per FLOAT / UINT channel; shape_dev: (geom, chan_words) on the device, if
    the caller has them; mode: uint8 [n] on the device, 1 PIZ, 0 stored raw, default all 1; sub_bits: bits per subsequence
    (PIZ_MIN_SUB_BITS .. 2^20, default PIZ_SUB_BITS); dst: a uint8 device tensor to write into (default: a new one, not cleared).
    Returns (dst, written int64 [n], status int32 [n]) on the device -- status 0, or an index into PIZ_REASONS, whose slot is left
    untouched -- and, with rounds=True, also an int32 [n, PIZ_ROUND_STATS] tensor: the synchronisation rounds each chunk took, then the
    subsequences that round 0, 1, ... decoded (round 0: all of them).  Stream-ordered, no host wait.
    stage_ms: a list that receives the two launches' device times (measurement: the call then waits)."""
    lib = _lib.load()
    geom = np.ascontiguousarray(geom, dtype=np.int32)
    words = np.ascontiguousarray(chan_words, dtype=np.int32)
    sub = 0 if sub_bits is None else int(sub_bits)
    ws_b = ctypes.c_int64(0)

    def sizes(src, s_host, d_host, n):
        if src.dim() != 1 or d_host.size != n + 1 or geom.shape != (n, 4) or words.ndim != 1:
            raise ValueError("piz_decode: expected src [size], two offset tables [n_chunks + 1], geom [n_chunks, 4] and chan_words [n]")
        src_b, dst_b = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(lib.shdr_piz_batch_sizes(_hptr(s_host), _hptr(d_host), _hptr(geom), _hptr(words), words.size, n, sub, ctypes.byref(src_b),
                                            ctypes.byref(dst_b), ctypes.byref(ws_b)), "shdr_piz_batch_sizes")
        return src_b.value, dst_b.value

    src, (s_host, s_dev), (d_host, d_dev), dst, mode, status, written = _slot_batch(
        "piz_decode", src, src_offsets, dst_offsets, src_offsets_dev, dst_offsets_dev, dst, mode, sizes)
    n, dev = s_host.size - 1, src.device
    geom_dev, words_dev = _shape_tables("piz_decode", geom, words, shape_dev, n, dev)
    rounds_dev = torch.empty((n, PIZ_ROUND_STATS), device=dev, dtype=torch.int32) if rounds else None
    ws = torch.empty(ws_b.value, device=dev, dtype=torch.uint8)
    with _stage_times(stage_ms, 2) as ms:
        _lib.check(lib.shdr_piz_batch(_ptr(src) if src.numel() else None, src.numel(), _hptr(s_host), _ptr(s_dev),
                                      _ptr(dst) if dst.numel() else None, dst.numel(), _hptr(d_host), _ptr(d_dev),
                                      _ptr(mode) if mode is not None else None, _hptr(geom), _ptr(geom_dev), _hptr(words), _ptr(words_dev),
                                      words.size, n, sub, _ptr(ws), ws.numel(), _ptr(status), _ptr(written),
                                      _ptr(rounds_dev) if rounds else None, _stream(), ms), "shdr_piz_batch")
    return (dst, written, status, rounds_dev) if rounds else (dst, written, status)


# ---------------------------------------------------------------------------
# OpenEXR PIZ chunks encoded (exr.py compression="piz"), see csrc/piz.h and csrc/piz_enc.hip.  UNPINNED against the OpenEXR library,
# like the decoder: no OpenEXR-built reader has opened what these write
# ---------------------------------------------------------------------------
PIZ_ENC_STAGES = 7                                    # SHDR_PIZ_ENC_STAGES
PIZ_ENC_STATS = 2                                     # SHDR_PIZ_ENC_STATS
PIZ_ENC_STAGE_NAMES = ("clear", "front", "hist", "code", "bits", "scan", "final")


def piz_encode_host(raw, width, rows, chan_words):
    """the planar scanline bytes of one chunk -> its PIZ bytes (libshdr's host encoder, csrc/piz.h: the rules the kernels run; byte
    for byte tests/piz_ref.py's encode_chunk).  chan_words: 1 per HALF channel, 2 per FLOAT / UINT channel, in name order.  The bytes
    are returned whatever their size: a chunk counts as coded only if len(result) < len(raw).  ValueError for a shape out of range
    or a size that is not the shape's."""
    lib = _lib.load()
    src = np.frombuffer(raw, dtype=np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw, dtype=np.uint8)
    words = np.ascontiguousarray(chan_words, dtype=np.int32)
    bound = lib.shdr_piz_encode_bound(int(width), int(rows), _hptr(words) if words.size else None, words.size)
    if bound < 0:
        raise ValueError(lib.shdr_last_error().decode())
    out = np.empty(bound, dtype=np.uint8)
    n = ctypes.c_int64(0)
    rc = lib.shdr_piz_encode_host(src.ctypes.data if src.size else None, src.size, int(width), int(rows), _hptr(words), words.size,
                                  _hptr(out), out.size, ctypes.byref(n))
    if rc != 0:
        raise ValueError(lib.shdr_last_error().decode())
    return out[:n.value].tobytes()


def piz_encode(planar, chunk_off, geom, chan_words, pad=0, front=0, stage_ms=None, chunk_off_dev=None, shape_dev=None, out=None, stats=False):
    """a batch of chunks PIZ-coded on the device (csrc/piz_enc.hip): byte for byte what piz_encode_host writes, and the same bytes on
    every run.  planar: uint8 device tensor, the chunks' planar scanlines (exr_pack(lines=32).planar); chunk_off: int64 [n + 1] (host
    array or tensor), chunk c is planar[chunk_off[c]:chunk_off[c + 1]]; geom: int32 [n, 4] host array (width, rows, first entry and
    number of entries in chan_words) and chan_words: int32 host array, as for piz_decode (shape_dev: their device copies).  Returns
    (bytes, out_offsets int64 [n + 1], coded uint8 [n]) on the device as deflate_huffman does: chunk c is stored at
    bytes[front + out_offsets[c] + pad : front + out_offsets[c + 1]] -- its PIZ bytes where coded[c], else (they would not be strictly
    fewer) its scanline bytes as they are.  pad: bytes left free in front of every stored chunk; front: bytes left free in front of all
    of them; out: a uint8 device tensor to store into (default: a new one, not cleared), at least front + the chunks' bytes + pad per
    chunk.  Stream-ordered, no host wait.  stage_ms: a list that receives the device times of PIZ_ENC_STAGE_NAMES (measurement: the
    call then waits).  stats=True (measurement): a fourth result, int32 [n, PIZ_ENC_STATS] on the device -- the symbols of every chunk's
    code and the ticks of the device's constant-rate counter that the one-lane merge of its code lengths took."""
    lib = _lib.load()
    planar = _chk(planar, "planar", torch.uint8)
    off_host, off_dev = _offsets_pair("piz_encode", "chunk_off", chunk_off, chunk_off_dev)
    n = off_host.size - 1
    geom = np.ascontiguousarray(geom, dtype=np.int32)
    words = np.ascontiguousarray(chan_words, dtype=np.int32)
    if planar.dim() != 1 or n < 1 or int(off_host[-1]) > planar.numel() or geom.shape != (n, 4) or words.ndim != 1:
        raise ValueError("piz_encode: expected planar [size], chunk_off [n_chunks + 1] that ends within it, geom [n_chunks, 4] and chan_words [n]")
    out_b, ws_b = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(lib.shdr_piz_encode_batch_sizes(_hptr(off_host), _hptr(geom), _hptr(words), words.size, n, int(pad), ctypes.byref(out_b),
                                               ctypes.byref(ws_b)), "shdr_piz_encode_batch_sizes")
    dev = planar.device
    if off_dev is None:
        off_dev = torch.from_numpy(off_host).to(dev)
    geom_dev, words_dev = _shape_tables("piz_encode", geom, words, shape_dev, n, dev)
    front = int(front)
    out, out_offsets, coded, ws = _store_buffers("piz_encode", out, front, out_b.value, ws_b.value, n, dev)
    stats_dev = torch.empty((n, PIZ_ENC_STATS), device=dev, dtype=torch.int32) if stats else None
    with _stage_times(stage_ms, PIZ_ENC_STAGES) as ms:
        _lib.check(lib.shdr_piz_encode_batch(_ptr(planar), _hptr(off_host), _ptr(off_dev), _hptr(geom), _ptr(geom_dev), _hptr(words),
                                             _ptr(words_dev), words.size, n, int(pad), out.data_ptr() + front, out_b.value, _ptr(out_offsets),
                                             _ptr(coded), _ptr(ws), ws.numel(), _ptr(stats_dev) if stats else None, _stream(), ms),
                   "shdr_piz_encode_batch")
    return (out, out_offsets, coded, stats_dev) if stats else (out, out_offsets, coded)


# ---------------------------------------------------------------------------
# JPEG scan regions unstuffed and laid out (jpeg.plan_device), see csrc/jpeg_scan.h and csrc/jpeg_scan.hip
# ---------------------------------------------------------------------------
JPEG_SCAN_IMAGE_BYTES, JPEG_SCAN_REPORT_BYTES = 40, 32          # shdr_jpeg_scan_image, shdr_jpeg_scan_report
JPEG_SCAN_TILE = 4096                                           # SHDR_JPEG_SCAN_TILE: raw bytes per workgroup


def _jpeg_scan_images(images, what):
    """(the descriptors as a contiguous host array, boundary slots, segments) of a structured array shaped like shdr_jpeg_scan_image
    (jpeg.SCAN_IMAGE_DTYPE)"""
    images = np.ascontiguousarray(images)
    if images.ndim != 1 or images.size == 0 or images.dtype.itemsize != JPEG_SCAN_IMAGE_BYTES or "seg_cap" not in (images.dtype.names or ()):
        raise ValueError("%s: images must be a non-empty array of jpeg.SCAN_IMAGE_DTYPE" % what)
    cap = images["seg_cap"].astype(np.int64)
    return images, int((cap - 1).sum()), int(cap.sum())


def jpeg_scan_host(src, images, seg_dword=None, seg_stride=1, arena_bytes=0):
    """libshdr's host twin of jpeg_scan / jpeg_compact (csrc/jpeg_scan.h, the rules the kernels run).  src: the bytes of the batch's
    scan regions; images: jpeg.SCAN_IMAGE_DTYPE [n].  Returns (report uint8 [n * 32]: view it as jpeg.SCAN_REPORT_DTYPE, bounds int64
    [sum(seg_cap - 1)], arena): arena is None without seg_dword (int32: entry s * seg_stride is the arena dword of segment s), else
    uint8 [arena_bytes]"""
    lib = _lib.load()
    src = np.ascontiguousarray(np.frombuffer(src, dtype=np.uint8) if isinstance(src, (bytes, bytearray, memoryview)) else src, dtype=np.uint8)
    images, n_bounds, n_segs = _jpeg_scan_images(images, "jpeg_scan_host")
    report = np.zeros(images.size * JPEG_SCAN_REPORT_BYTES, dtype=np.uint8)
    bounds = np.zeros(max(n_bounds, 1), dtype=np.int64)
    arena = None
    if seg_dword is not None:
        seg_dword = np.ascontiguousarray(seg_dword, dtype=np.int32).reshape(-1)
        arena = np.zeros(max(int(arena_bytes), 1), dtype=np.uint8)
    _lib.check(lib.shdr_jpeg_scan_host(_hptr(src) if src.size else None, src.size, _hptr(images), images.size, _hptr(report), _hptr(bounds),
                                       n_bounds, _hptr(seg_dword) if seg_dword is not None else None, int(seg_stride),
                                       seg_dword.size // int(seg_stride) if seg_dword is not None else 0,
                                       _hptr(arena) if arena is not None else None, int(arena_bytes)), "shdr_jpeg_scan_host")
    return report, bounds[:n_bounds], None if arena is None else arena[:int(arena_bytes)]


def jpeg_scan(src, images, images_dev=None, stage_ms=None):
    """the scan call on the device (csrc/jpeg_scan.hip): src uint8 device tensor, the regions at images["offset"] (multiples of 16);
    images: jpeg.SCAN_IMAGE_DTYPE [n] on the host (validated by libshdr), images_dev its device copy as uint8 (made here if None).
    Returns (result, workspace, images_dev): result is ONE uint8 device tensor, n reports of 32 bytes (jpeg.SCAN_REPORT_DTYPE) followed by
    the int64 boundaries [sum(seg_cap - 1)], so that one copy brings both back; workspace and images_dev are what jpeg_compact wants.
    Stream-ordered, no host wait.  stage_ms: a list that receives the device time of the call (measurement: the call then waits)."""
    lib = _lib.load()
    src = _chk(src, "src", torch.uint8)
    images, n_bounds, _ = _jpeg_scan_images(images, "jpeg_scan")
    dev, n = src.device, images.size
    if images_dev is None:
        images_dev = torch.from_numpy(images.view(np.uint8)).to(dev)
    if _chk(images_dev, "images_dev", torch.uint8).numel() != n * JPEG_SCAN_IMAGE_BYTES:
        raise ValueError("jpeg_scan: images_dev is not a copy of images")
    n_tiles = int((-(-images["length"].astype(np.int64) // JPEG_SCAN_TILE)).sum())
    ws_bytes = lib.shdr_jpeg_scan_workspace_bytes(n, n_tiles)
    if ws_bytes < 0:
        raise ValueError(lib.shdr_last_error().decode())
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    result = torch.empty(n * JPEG_SCAN_REPORT_BYTES + 8 * n_bounds, device=dev, dtype=torch.uint8)
    with _stage_times(stage_ms, 1) as ms:
        _lib.check(lib.shdr_jpeg_scan(_ptr(src) if src.numel() else None, src.numel(), _hptr(images), _ptr(images_dev), n, _ptr(result),
                                      ctypes.c_void_p(result.data_ptr() + n * JPEG_SCAN_REPORT_BYTES) if n_bounds else None, n_bounds,
                                      _ptr(ws), _stream(), ms), "shdr_jpeg_scan")
    return result, ws, images_dev


def jpeg_compact(src, images, images_dev, result, workspace, seg_dword, seg_stride, arena_bytes, stage_ms=None):
    """the compaction call: src, images, images_dev as for jpeg_scan, result and workspace what it returned for them; seg_dword: int32
    device tensor whose entry s * seg_stride is the arena dword of segment s (the uploaded `segs` table with seg_stride 6 will do).
    Returns the arena, uint8 [arena_bytes] on the device: FF, then every kept byte at its place.  Stream-ordered, no host wait."""
    lib = _lib.load()
    src = _chk(src, "src", torch.uint8)
    images, n_bounds, n_segs = _jpeg_scan_images(images, "jpeg_compact")
    n, seg_stride, arena_bytes = images.size, int(seg_stride), int(arena_bytes)
    seg_dword = _chk(seg_dword, "seg_dword", torch.int32)
    if _chk(result, "result", torch.uint8).numel() != n * JPEG_SCAN_REPORT_BYTES + 8 * n_bounds or \
            _chk(images_dev, "images_dev", torch.uint8).numel() != n * JPEG_SCAN_IMAGE_BYTES:
        raise ValueError("jpeg_compact: result and images_dev must be those of jpeg_scan for these images")
    if seg_stride < 1 or seg_dword.numel() < n_segs * seg_stride or arena_bytes < 0:
        raise ValueError("jpeg_compact: seg_dword must hold %d segments of stride %d" % (n_segs, seg_stride))
    _chk(workspace, "workspace", torch.uint8)
    arena = torch.empty(arena_bytes, device=src.device, dtype=torch.uint8)
    with _stage_times(stage_ms, 1) as ms:
        _lib.check(lib.shdr_jpeg_compact(_ptr(src) if src.numel() else None, src.numel(), _hptr(images), _ptr(images_dev), n,
                                         ctypes.c_void_p(result.data_ptr() + n * JPEG_SCAN_REPORT_BYTES) if n_bounds else None, n_bounds,
                                         _ptr(seg_dword), seg_stride, seg_dword.numel() // seg_stride, _ptr(arena) if arena_bytes else None,
                                         arena_bytes, _ptr(workspace), _stream(), ms), "shdr_jpeg_compact")
    return arena


# ---------------------------------------------------------------------------
# baseline-JPEG writer (jpeg.encode), see csrc/jpeg_enc.hip and csrc/jpeg_enc.h
# ---------------------------------------------------------------------------
JPEG_ENC_IMAGE_DTYPE = np.dtype([(name, np.int32) for name in ("height", "width", "layout", "quality", "restart", "reserved")])   # shdr_jpeg_enc_image
JPEG_ENC_HEADER_MAX = 640                                       # SHDR_JPEG_ENC_HEADER_MAX
JPEG_ENC_STAGES = 7                                             # SHDR_JPEG_ENC_STAGES
JPEG_ENC_STAGE_NAMES = ("transform", "bits", "scan_segments", "bit_stream", "ff_count_scan", "sizes_scan", "final")
JPEG_ENC_OUT_OF_RANGE = 1                                       # SHDR_JPEG_ENC_OUT_OF_RANGE
JPEG_ENC_LAYOUTS = {"444": 0, "422": 1, "420": 2}
JPEG_ENC_GUARD = 0xA5                                           # what the guard bytes of jpeg_encode(..., guard=) hold


def jpeg_enc_images(shapes, quality=75, subsampling="420", restart_interval=0):
    """the descriptors (JPEG_ENC_IMAGE_DTYPE [n]) of images of `shapes` [(H, W)]; quality, subsampling ("444" | "422" | "420") and
    restart_interval (MCUs, 0 .. 65535): one value for all images or one per image.  ValueError for anything outside the writer's scope."""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    n = len(shapes)
    if n == 0:
        raise ValueError("jpeg_encode: no images")

    def per_image(value, name):
        values = list(value) if isinstance(value, (list, tuple, np.ndarray)) else [value] * n
        if len(values) != n:
            raise ValueError("jpeg_encode: %d values of %s for %d images" % (len(values), name, n))
        return values
    images = np.zeros(n, dtype=JPEG_ENC_IMAGE_DTYPE)
    for i, (shape, q, sub, rst) in enumerate(zip(shapes, per_image(quality, "quality"), per_image(subsampling, "subsampling"),
                                                 per_image(restart_interval, "restart_interval"))):
        if len(shape) != 2 or not (1 <= shape[0] <= 65535 and 1 <= shape[1] <= 65535):
            raise ValueError("jpeg_encode: image %d is %s: H and W must be 1 .. 65535" % (i, shape))
        if str(sub) not in JPEG_ENC_LAYOUTS:
            raise ValueError("jpeg_encode: subsampling must be '444', '422' or '420', got %r" % (sub,))
        if isinstance(q, bool) or int(q) != q or not 1 <= int(q) <= 100:
            raise ValueError("jpeg_encode: quality must be an integer 1 .. 100, got %r" % (q,))
        if isinstance(rst, bool) or int(rst) != rst or not 0 <= int(rst) <= 65535:
            raise ValueError("jpeg_encode: restart_interval must be an integer 0 .. 65535 (MCUs), got %r" % (rst,))
        images[i] = (shape[0], shape[1], JPEG_ENC_LAYOUTS[str(sub)], int(q), int(rst), 0)
    return images


def _jpeg_enc_image(image, what):
    image = np.ascontiguousarray(image)
    if image.dtype != JPEG_ENC_IMAGE_DTYPE or image.size != 1:
        raise ValueError("%s: expected one descriptor of JPEG_ENC_IMAGE_DTYPE (jpeg_enc_images)" % what)
    return image.reshape(1)


def _jpeg_enc_fail(lib, n):
    if n < 0:
        raise ValueError(lib.shdr_last_error().decode())
    return n


def jpeg_encode_blocks(image):
    """(blocks of the image's coefficient arena, an upper bound of its file in bytes)"""
    lib = _lib.load()
    image = _jpeg_enc_image(image, "jpeg_encode_blocks")
    bound = ctypes.c_int64(0)
    return _jpeg_enc_fail(lib, lib.shdr_jpeg_encode_blocks(_hptr(image), ctypes.byref(bound))), bound.value


def jpeg_encode_header_host(image):
    """the bytes from SOI to the end of the SOS header"""
    lib = _lib.load()
    image = _jpeg_enc_image(image, "jpeg_encode_header_host")
    out = np.zeros(JPEG_ENC_HEADER_MAX, dtype=np.uint8)
    return out[:_jpeg_enc_fail(lib, lib.shdr_jpeg_encode_header_host(_hptr(image), _hptr(out)))].tobytes()


def jpeg_encode_transform_host(rgb, image):
    """first stage of the host twin: uint8 [H, W, 3] -> int16 [blocks, 64] (zig-zag order, MCU scan order, dummy blocks included)"""
    lib = _lib.load()
    image = _jpeg_enc_image(image, "jpeg_encode_transform_host")
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.shape != (int(image["height"][0]), int(image["width"][0]), 3):
        raise ValueError("jpeg_encode_transform_host: expected uint8 [H, W, 3] of the descriptor's size, got %s %s" % (rgb.dtype, rgb.shape))
    blocks, _ = jpeg_encode_blocks(image)
    coef = np.zeros((blocks, 64), dtype=np.int16)
    _jpeg_enc_fail(lib, lib.shdr_jpeg_encode_transform_host(_hptr(rgb), _hptr(image), _hptr(coef), blocks))
    return coef


def jpeg_encode_entropy_host(coef, image, capacity=None, guard=0):
    """second stage of the host twin: int16 [blocks, 64] -> the scan's bytes (stuffed segments and RSTn markers; no header, no EOI).
    capacity: room of the output (default: the bound); guard: with it, returns (bytes, the guard bytes behind the room)"""
    lib = _lib.load()
    image = _jpeg_enc_image(image, "jpeg_encode_entropy_host")
    coef = np.ascontiguousarray(coef)
    if coef.dtype != np.int16 or coef.ndim != 2 or coef.shape[1] != 64:
        raise ValueError("jpeg_encode_entropy_host: expected int16 [blocks, 64]")
    cap = jpeg_encode_blocks(image)[1] if capacity is None else int(capacity)
    out = np.full(max(cap, 0) + int(guard), JPEG_ENC_GUARD, dtype=np.uint8)
    try:
        n = _jpeg_enc_fail(lib, lib.shdr_jpeg_encode_entropy_host(_hptr(coef), coef.shape[0], _hptr(image), _hptr(out), cap))
    except ValueError as e:
        if guard:
            e.guard = out[max(cap, 0):].copy()
        raise
    return (out[:n].tobytes(), out[cap:].copy()) if guard else out[:n].tobytes()


def jpeg_encode_host(rgb, image, capacity=None, guard=0):
    """the host twin: the complete file of uint8 [H, W, 3]; capacity, guard: as jpeg_encode_entropy_host"""
    lib = _lib.load()
    image = _jpeg_enc_image(image, "jpeg_encode_host")
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint8 or rgb.shape != (int(image["height"][0]), int(image["width"][0]), 3):
        raise ValueError("jpeg_encode_host: expected uint8 [H, W, 3] of the descriptor's size, got %s %s" % (rgb.dtype, rgb.shape))
    cap = jpeg_encode_blocks(image)[1] if capacity is None else int(capacity)
    out = np.full(max(cap, 0) + int(guard), JPEG_ENC_GUARD, dtype=np.uint8)
    try:
        n = _jpeg_enc_fail(lib, lib.shdr_jpeg_encode_host(_hptr(rgb), _hptr(image), _hptr(out), cap))
    except ValueError as e:
        if guard:
            e.guard = out[max(cap, 0):].copy()
        raise
    return (out[:n].tobytes(), out[cap:].copy()) if guard else out[:n].tobytes()


def _jpeg_enc_pixels(pixels, what):
    """(flat pixels, [(H, W)]) of one [H, W, 3] or [N, H, W, 3] device tensor (used as it is) or a list of [H, W, 3] tensors (packed back to
    back on the device); uint8, or float32 in [0, 1]"""
    def chk(t):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in (torch.uint8, torch.float32) and t.dim() in (3, 4) and t.shape[-1] == 3):
            raise TypeError("%s: expected uint8 or float32 RGB device tensors [H, W, 3] or [N, H, W, 3]" % what)
        if t.numel() == 0:
            raise ValueError("%s: an image has no pixels: %s" % (what, tuple(t.shape)))
        return t.contiguous()
    if isinstance(pixels, (list, tuple)):
        if not pixels:
            raise ValueError("%s: no images" % what)
        imgs = [chk(t) for t in pixels]
        if any(t.dim() != 3 for t in imgs) or any(t.dtype != imgs[0].dtype for t in imgs):
            raise TypeError("%s: a list holds single images [H, W, 3] of one dtype" % what)
        flat = imgs[0].reshape(-1) if len(imgs) == 1 else torch.cat([t.reshape(-1) for t in imgs])
        return flat, [tuple(t.shape[:2]) for t in imgs]
    t = chk(pixels)
    return t.reshape(-1), [tuple(t.shape[-3:-1])] * (1 if t.dim() == 3 else t.shape[0])


def _jpeg_enc_run(what, images, dev, stage_ms, guard, info, call, buffers=None):
    """the buffers and the call shared by jpeg_encode and jpeg_encode_entropy: call(lib, images_dev, out, cap, offsets, status, ws, ms).
    buffers: a dict in which output and workspace are kept from call to call and grown when needed (both are sized for the worst
    case, hundreds of MB for a 12-Mpixel image) -- for a caller that has finished with the previous call's output"""
    lib = _lib.load()
    n = images.size
    out_b, blocks, ws_b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.shdr_jpeg_encode_batch_sizes(_hptr(images), n, ctypes.byref(out_b), ctypes.byref(blocks), ctypes.byref(ws_b))
    if rc != 0:
        raise ValueError(lib.shdr_last_error().decode())
    guard = (int(guard) + 15) // 16 * 16
    fill = (lambda size: torch.full((size,), JPEG_ENC_GUARD, device=dev, dtype=torch.uint8)) if guard else \
        (lambda size: torch.empty(size, device=dev, dtype=torch.uint8))
    if buffers is not None and not guard:
        kept = buffers.get("raw")
        if kept is None or kept[0].device != dev or kept[0].numel() < out_b.value or kept[1].numel() < ws_b.value:
            buffers["raw"] = kept = (fill(out_b.value), fill(ws_b.value))
        out_raw, ws_raw = kept
    else:
        out_raw, ws_raw = fill(out_b.value + 2 * guard), fill(ws_b.value + 2 * guard)
    out, ws = out_raw[guard:guard + out_b.value], ws_raw[guard:guard + ws_b.value]
    offsets = torch.empty(n + 1, device=dev, dtype=torch.int64)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    images_dev = torch.from_numpy(images.view(np.uint8).copy()).to(dev)
    with _stage_times(stage_ms, JPEG_ENC_STAGES) as ms:
        _lib.check(call(lib, images_dev, out, out_b.value, offsets, status, ws, ms, blocks.value), what)
    if info is not None:
        info.update(out_raw=out_raw, workspace_raw=ws_raw, guard=guard, blocks=blocks.value, out_bytes=out_b.value, workspace_bytes=ws_b.value)
    return out, offsets, status


def jpeg_encode(pixels, images, stage_ms=None, guard=0, info=None, buffers=None):
    """Baseline-JPEG files of a batch of RGB images, written on the device (csrc/jpeg_enc.hip): byte for byte what the host twin
    jpeg_encode_host -- and PIL, for the same quality, subsampling and restart_marker_blocks -- writes.  pixels: uint8, or float32 in
    [0, 1] (quantised as jpeg_round_trip does), one device tensor [H, W, 3] or [N, H, W, 3] (no copy) or a list of [H, W, 3] tensors of
    different sizes; images: their descriptors (jpeg_enc_images).  Returns (bytes uint8, offsets int64 [n + 1], status int32 [n]) on the
    device: file i is bytes[offsets[i]:offsets[i + 1]]; status[i] != 0 (JPEG_ENC_OUT_OF_RANGE) leaves file i empty.  Stream-ordered, no
    host wait.  stage_ms: a list that receives the device times of the JPEG_ENC_STAGE_NAMES (measurement: the call then waits); guard:
    bytes of JPEG_ENC_GUARD around the output and the workspace, returned through `info` (a dict) for inspection; buffers: a dict
    that keeps output and workspace for the next call (the returned bytes are then valid until that call)."""
    flat, shapes = _jpeg_enc_pixels(pixels, "jpeg_encode")
    images = np.ascontiguousarray(images)
    if images.dtype != JPEG_ENC_IMAGE_DTYPE or images.ndim != 1 or [(int(a), int(b)) for a, b in zip(images["height"], images["width"])] != \
            [(int(a), int(b)) for a, b in shapes]:
        raise ValueError("jpeg_encode: images must be the descriptors (jpeg_enc_images) of exactly these pixels")
    lib = _lib.load()
    headers = np.zeros((images.size, JPEG_ENC_HEADER_MAX), dtype=np.uint8)
    for i in range(images.size):
        _jpeg_enc_fail(lib, lib.shdr_jpeg_encode_header_host(_hptr(images[i:i + 1]), _hptr(headers[i])))
    headers_dev = torch.from_numpy(headers).to(flat.device)
    ptype = 0 if flat.dtype == torch.uint8 else 1

    def call(lib, images_dev, out, cap, offsets, status, ws, ms, blocks):
        return lib.shdr_jpeg_encode_batch(_ptr(flat), ptype, _hptr(images), _ptr(images_dev), _hptr(headers), _ptr(headers_dev), images.size,
                                          _ptr(out), cap, _ptr(offsets), _ptr(status), _ptr(ws), _stream(), ms)
    return _jpeg_enc_run("shdr_jpeg_encode_batch", images, flat.device, stage_ms, guard, info, call, buffers)


def jpeg_encode_entropy(coef, images, stage_ms=None, guard=0, info=None):
    """the entropy stages alone: coef int16 device tensor [blocks, 64], the images' arenas back to back (jpeg_encode_transform_host's
    layout); returns what jpeg_encode returns, file i being the scan jpeg_encode_entropy_host writes (no header, no EOI)"""
    coef = _chk(coef, "coef", torch.int16)
    images = np.ascontiguousarray(images)
    if images.dtype != JPEG_ENC_IMAGE_DTYPE or images.ndim != 1 or coef.dim() != 2 or coef.shape[1] != 64:
        raise ValueError("jpeg_encode_entropy: expected coef int16 [blocks, 64] and descriptors (jpeg_enc_images)")

    def call(lib, images_dev, out, cap, offsets, status, ws, ms, blocks):
        return lib.shdr_jpeg_encode_entropy_batch(_ptr(coef), coef.shape[0], _hptr(images), _ptr(images_dev), images.size, _ptr(out), cap,
                                                  _ptr(offsets), _ptr(status), _ptr(ws), _stream(), ms)
    return _jpeg_enc_run("shdr_jpeg_encode_entropy_batch", images, coef.device, stage_ms, guard, info, call)


# ---------------------------------------------------------------------------
# PNG writer (png.encode), see csrc/png_enc.hip and csrc/png.h
# ---------------------------------------------------------------------------
PNG_SEGMENT = 65520                                             # SHDR_PNG_SEGMENT
PNG_FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")   # SHDR_PNG_FILTER_*: the index is the value
PNG_DEFLATES = ("huffman", "lz")                                # SHDR_PNG_DEFLATE_*
PNG_STAGE_NAMES = ("filter", "deflate_sizes", "deflate_scan", "deflate_blocks", "frame_crc")   # SHDR_PNG_STAGES


def _png_options(what, filter, deflate):
    if filter not in PNG_FILTERS:
        raise ValueError("%s: filter must be one of %s, got %r" % (what, ", ".join(PNG_FILTERS), filter))
    if deflate not in PNG_DEFLATES:
        raise ValueError("%s: deflate must be 'lz' or 'huffman', got %r" % (what, deflate))
    return PNG_FILTERS.index(filter), PNG_DEFLATES.index(deflate)


def _png_host_image(image, what):
    """uint8 [H, W] or [H, W, C] host array -> contiguous [H, W, C], C in (1, 3, 4), no empty dimension"""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise TypeError("%s: expected uint8 pixels, got %s" % (what, a.dtype))
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError("%s: expected [H, W] or [H, W, C] with C = 1 (grey), 3 (RGB) or 4 (RGBA), got %s" % (what, a.shape))
    if 0 in a.shape:
        raise ValueError("%s: an image has no pixels: %s" % (what, a.shape))
    return np.ascontiguousarray(a)


def crc32(data, crc=0):
    """CRC-32 (IEEE: zlib.crc32) of bytes by the libshdr host routine"""
    src = np.frombuffer(bytes(data), dtype=np.uint8)
    return int(_lib.load().shdr_crc32(_hptr(src) if src.size else None, src.size, crc))


def png_filter_host(image, filter="adaptive"):
    """the filtered stream of one uint8 image [H, W] or [H, W, C] (bytes: per row the filter type and W C filtered bytes), by the
    libshdr host routine (csrc/png.h)"""
    lib = _lib.load()
    a = _png_host_image(image, "png_filter_host")
    f, _ = _png_options("png_filter_host", filter, "lz")
    h, w, c = a.shape
    out = np.empty(h * (w * c + 1), dtype=np.uint8)
    n = lib.shdr_png_filter_host(_hptr(a), h, w, c, f, _hptr(out), out.size)
    if n < 0:
        raise ValueError(lib.shdr_last_error().decode())
    return out[:n].tobytes()


def png_bound(h, w, c):
    """no PNG file of an H x W x C image is larger (every segment stored)"""
    stream = h * (w * c + 1)
    return 8 + 25 + 12 + 6 + stream + 17 * (-(-stream // PNG_SEGMENT))


def png_encode_host(image, filter="adaptive", deflate="lz", capacity=None):
    """the host twin: the complete PNG file (bytes) of one uint8 image [H, W] or [H, W, C]; capacity: the size of the destination
    (default: png_bound), a smaller one than the file raises ValueError"""
    lib = _lib.load()
    a = _png_host_image(image, "png_encode_host")
    f, d = _png_options("png_encode_host", filter, deflate)
    h, w, c = a.shape
    cap = png_bound(h, w, c) if capacity is None else int(capacity)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    n = lib.shdr_png_encode_host(_hptr(a), h, w, c, f, d, _hptr(out), cap)
    if n < 0:
        raise ValueError(lib.shdr_last_error().decode())
    return out[:n].tobytes()


def png_encode(pixels, shapes, filter="adaptive", deflate="lz", stage_ms=None, buffers=None):
    """PNG files of a batch of 8-bit images, written on the device (csrc/png_enc.hip): byte for byte what png_encode_host writes.
    pixels: uint8 device tensor, the images' [H, W, C] pixels back to back; shapes: their (H, W, C).  Returns (bytes uint8,
    offsets int64 [n + 1]) on the device: file i is bytes[offsets[i]:offsets[i + 1]].  Stream-ordered, no host wait.  stage_ms: a
    list that receives the device times of the PNG_STAGE_NAMES (measurement: the call then waits); buffers: a dict that keeps output
    and workspace for the next call and grows them when needed (both are sized for the worst case; with deflate="lz" the workspace
    holds 4 bytes per filtered byte) -- the returned bytes are then valid until that call."""
    lib = _lib.load()
    pixels = _chk(pixels, "pixels", torch.uint8)
    f, d = _png_options("png_encode", filter, deflate)
    images = np.zeros((len(shapes), 4), dtype=np.int32)
    for i, shape in enumerate(shapes):
        if len(shape) != 3 or shape[2] not in (1, 3, 4) or min(shape) < 1:
            raise ValueError("png_encode: image %d is %s: expected (H, W, C) with C = 1, 3 or 4 and no empty dimension" % (i, tuple(shape)))
        images[i, :3] = shape
    n = images.shape[0]
    pix_b, out_b, segs, ws_b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.shdr_png_encode_batch_sizes(_hptr(images), n, d, ctypes.byref(pix_b), ctypes.byref(out_b), ctypes.byref(segs), ctypes.byref(ws_b))
    if rc != 0:
        raise ValueError(lib.shdr_last_error().decode())
    if pixels.dim() != 1 or pixels.numel() != pix_b.value:
        raise ValueError("png_encode: pixels must be the %d bytes of these shapes back to back, got %s" % (pix_b.value, tuple(pixels.shape)))
    dev = pixels.device
    kept = buffers.get("raw") if buffers is not None else None
    if kept is None or kept[0].device != dev or kept[0].numel() < out_b.value or kept[1].numel() < ws_b.value:
        kept = (torch.empty(out_b.value, device=dev, dtype=torch.uint8), torch.empty(ws_b.value, device=dev, dtype=torch.uint8))
        if buffers is not None:
            buffers["raw"] = kept
    out, ws = kept[0][:out_b.value], kept[1][:ws_b.value]
    offsets = torch.empty(n + 1, device=dev, dtype=torch.int64)
    images_dev = torch.from_numpy(images).to(dev)
    with _stage_times(stage_ms, len(PNG_STAGE_NAMES)) as ms:
        _lib.check(lib.shdr_png_encode_batch(_ptr(pixels), _hptr(images), _ptr(images_dev), n, f, d, _ptr(out), out_b.value, _ptr(offsets),
                                             _ptr(ws), _stream(), ms), "shdr_png_encode_batch")
    return out, offsets


EXR_HALF, EXR_FLOAT = 1, 2


def _exr_batch(images, what):
    """(flat float32 pixels, host shape table int32 [n, 2]) of `images`: one [H, W, 3] or [N, H, W, 3] tensor (used as it is, no copy)
    or a list of [H, W, 3] tensors of different sizes (packed back to back on the device): the convention of _rle_batch"""
    def chk(t):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise TypeError("%s: expected float32 device tensors [H, W, 3] or [N, H, W, 3]" % what)
        if t.dtype != torch.float32 or t.dim() not in (3, 4) or t.shape[-1] != 3:
            raise ValueError("%s: expected float32 images [H, W, 3] or [N, H, W, 3], got %s %s" % (what, t.dtype, tuple(t.shape)))
        if t.numel() == 0:
            raise ValueError("%s: an image has no pixels: %s" % (what, tuple(t.shape)))
        return _d(t).contiguous()
    if isinstance(images, (list, tuple)):
        if not images:
            raise ValueError("%s: no images" % what)
        imgs = [chk(t) for t in images]
        if any(t.dim() != 3 for t in imgs):
            raise ValueError("%s: a list holds single images [H, W, 3]" % what)
        shapes = np.array([t.shape[:2] for t in imgs], dtype=np.int32)
        flat = imgs[0].reshape(-1) if len(imgs) == 1 else torch.cat([t.reshape(-1) for t in imgs])
        return flat, shapes
    t = chk(images)
    n = 1 if t.dim() == 3 else t.shape[0]
    return t.reshape(-1), np.tile(np.array(t.shape[-3:-1], dtype=np.int32), (n, 1))


ExrPacked = collections.namedtuple("ExrPacked", "planar predicted chunk_off chunk_off_dev table table_dev shapes lines")
"""planar / predicted: uint8 device tensors [bytes] (predicted None unless asked for); chunk_off: host int64 [n_chunks + 1], chunk c is
bytes [chunk_off[c], chunk_off[c + 1]) of both (chunk_off_dev: its device copy); table: host int64 [3, n_images + 1] (first chunk, first
pixel, H * 2^32 + W of every image; table_dev: its device copy); shapes: host int32 [n_images, 2]; lines: scanlines per chunk"""


def exr_pack(images, pixel_type=EXR_HALF, lines=16, reverse_channels=False, saturate=True, predict=True):
    """float32 images -> OpenEXR scanline bytes on the device, one launch for the whole batch (csrc/exr_write.hip).  images: one
    [H, W, 3], one [N, H, W, 3] or a list of [H, W, 3] device tensors.  Every chunk (`lines` scanlines: 32 for PIZ, 16 for ZIP, 1 for ZIPS / NONE)
    holds per scanline W samples of B, then G, then R, HALF (numpy's astype(float16); saturate: finite values beyond +-65504 become
    +-65504 first) or FLOAT.  reverse_channels: channel 0 of the input is blue (the networks' order).  predict: also the interleaved,
    delta-coded bytes of every chunk, which ZIP / ZIPS deflate.  Returns an ExrPacked."""
    lib = _lib.load()
    flat, shapes = _exr_batch(images, "exr_pack")
    n = shapes.shape[0]
    n_chunks, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
    args = (_hptr(shapes), n, int(pixel_type), int(lines))
    _lib.check(lib.shdr_exr_pack_sizes(*args, ctypes.byref(n_chunks), ctypes.byref(nbytes), None, None), "shdr_exr_pack_sizes")
    tabs = np.empty(3 * (n + 1) + n_chunks.value + 1, dtype=np.int64)           # one array, one upload
    table, chunk_off = tabs[:3 * (n + 1)], tabs[3 * (n + 1):]
    _lib.check(lib.shdr_exr_pack_sizes(*args, None, None, _hptr(table), _hptr(chunk_off)), "shdr_exr_pack_sizes")
    dev = flat.device
    tabs_dev = torch.from_numpy(tabs).to(dev)
    table_dev, chunk_off_dev = tabs_dev[:3 * (n + 1)], tabs_dev[3 * (n + 1):]
    planar = torch.empty(nbytes.value, device=dev, dtype=torch.uint8)
    predicted = torch.empty(nbytes.value, device=dev, dtype=torch.uint8) if predict else None
    _lib.check(lib.shdr_exr_pack_f32(_ptr(flat), _hptr(shapes), n, int(pixel_type), int(lines), int(bool(reverse_channels)),
                                     int(bool(saturate)), _ptr(table_dev), _ptr(chunk_off_dev), _ptr(planar),
                                     _ptr(predicted) if predict else None, _stream()), "shdr_exr_pack_f32")
    return ExrPacked(planar, predicted, chunk_off, chunk_off_dev, table.reshape(3, n + 1), table_dev, shapes, int(lines))


def exr_finish_chunks(out, out_offsets, packed, header_len):
    """chunk headers (int32 y, int32 size) and uint64 offset tables into `out` of deflate_huffman / piz_encode(..., pad=8, front=8 * n_chunks):
    the tables of all images fill the front, image after image; header_len: the bytes of every file in front of its table"""
    lib = _lib.load()
    n, n_chunks = packed.shapes.shape[0], packed.chunk_off.size - 1
    hl = torch.from_numpy(np.ascontiguousarray(header_len, dtype=np.int64)).to(out.device)
    if hl.numel() != n or out.numel() < 8 * n_chunks or out_offsets.numel() != n_chunks + 1:
        raise ValueError("exr_finish_chunks: the buffers do not belong to this batch")
    _lib.check(lib.shdr_exr_finish_chunks(out.data_ptr() + 8 * n_chunks, _ptr(out), _ptr(out_offsets), _ptr(packed.table_dev), _ptr(hl), n,
                                          n_chunks, packed.lines, _stream()), "shdr_exr_finish_chunks")
    return out


# ---------------------------------------------------------------------------
# HDR-Real image folders (hdr_real.py), see csrc/hdr_real.hip
# ---------------------------------------------------------------------------
def _host_table(a, name, dtype):
    """a host table [n, 3] as the C ABI wants it: contiguous, of the given dtype (values that do not fit are refused, not wrapped)"""
    arr = np.ascontiguousarray(a)
    if arr.ndim != 2 or arr.shape[1] != 3 or arr.dtype.kind not in "iu":
        raise ValueError("%s: expected an integer table [n, 3]" % name)
    if arr.dtype == dtype:
        return arr
    out = arr.astype(dtype)
    if not np.array_equal(out, arr):
        raise ValueError("%s: values do not fit %s" % (name, np.dtype(dtype).name))
    return out


def _pair_tables(ldr, hdr, images, images_dev, patches, patches_dev, what):
    ldr = _chk(ldr, "ldr", torch.uint8)
    hdr = _chk(hdr, "hdr")
    if ldr.numel() != hdr.numel() or ldr.numel() % 3:
        raise ValueError("%s: the arenas must hold the same pixels, [arena_pixels, 3] each" % what)
    images, patches = _host_table(images, "images", np.int64), _host_table(patches, "patches", np.int32)
    images_dev = _chk(images_dev, "images_dev", torch.int64)
    patches_dev = _chk(patches_dev, "patches_dev", torch.int32)
    if tuple(images_dev.shape) != images.shape or tuple(patches_dev.shape) != patches.shape:
        raise ValueError("%s: a device table is not the shape of its host table" % what)
    return ldr, hdr, images, images_dev, patches, patches_dev


def _hptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def pair_patch_stats(ldr, hdr, images, images_dev, patches, patches_dev, size):
    """(count int32 [n_patches], mean float32 [n_patches]) of every size x size patch of the resident pairs: the extreme-pixel
    count of convert_to_tf_record.py:54-55 and the float64-summed HDR mean.  ldr uint8 / hdr float32 arenas [arena_pixels, 3];
    images int64 [n, 3] (first pixel, H, W), patches int32 [p, 3] (image, h1, w1): host arrays, which libshdr validates before it
    launches, and their device copies, which the kernel reads (include/shdr.h)."""
    lib = _lib.load()
    ldr, hdr, images, images_dev, patches, patches_dev = _pair_tables(ldr, hdr, images, images_dev, patches, patches_dev,
                                                                      "pair_patch_stats")
    n = patches.shape[0]
    count = torch.empty(n, device=hdr.device, dtype=torch.int32)
    mean = torch.empty(n, device=hdr.device, dtype=torch.float32)
    _lib.check(lib.shdr_pair_patch_stats(_ptr(ldr), _ptr(hdr), ldr.numel() // 3, _hptr(images), _ptr(images_dev), images.shape[0],
                                         _hptr(patches), _ptr(patches_dev), n, int(size), _ptr(count), _ptr(mean), _stream()),
               "shdr_pair_patch_stats")
    return count, mean


def pair_patch_gather(ldr, hdr, images, images_dev, patches, patches_dev, mean, samples, size):
    """(ref_LDR, ref_HDR) float32 [b, size, size, 3] for samples int32 [b, 3] (patch, flip, rot) -- a host array: it is validated by
    libshdr, copied to the device through pinned memory here, and one launch crops, flips, rotates and normalises both patches
    (LDR / 255, HDR / (1e-6 + mean[patch]) * 0.5)."""
    lib = _lib.load()
    ldr, hdr, images, images_dev, patches, patches_dev = _pair_tables(ldr, hdr, images, images_dev, patches, patches_dev,
                                                                      "pair_patch_gather")
    mean = _chk(mean, "mean")
    if mean.numel() != patches.shape[0]:
        raise ValueError("pair_patch_gather: one mean per patch")
    samples = _host_table(samples, "samples", np.int32)
    b = samples.shape[0]
    samples_dev = torch.from_numpy(samples).pin_memory().to(hdr.device, non_blocking=True) if b else None
    shape = (b, int(size), int(size), 3) if b > 0 and size > 0 else (0,)
    out_ldr = torch.empty(shape, device=hdr.device, dtype=torch.float32)
    out_hdr = torch.empty(shape, device=hdr.device, dtype=torch.float32)
    _lib.check(lib.shdr_pair_patch_gather_f32(_ptr(ldr), _ptr(hdr), ldr.numel() // 3, _hptr(images), _ptr(images_dev), images.shape[0],
                                              _hptr(patches), _ptr(patches_dev), patches.shape[0], _ptr(mean), _hptr(samples),
                                              None if samples_dev is None else _ptr(samples_dev), b, int(size), _ptr(out_ldr),
                                              _ptr(out_hdr), _stream()), "shdr_pair_patch_gather_f32")
    return out_ldr, out_hdr


# ---------------------------------------------------------------------------
# validation metrics (csrc/metrics.hip; the public layer is metrics.py)
# ---------------------------------------------------------------------------
METRICS_TILE = (16, 32)        # SSIM windows per block of shdr_hdr_metrics_f32 (SHDR_METRICS_TILE_H x _W, include/shdr.h)


def _pair(pred, gt, what):
    pred, gt = _chk(_d(pred), "pred"), _chk(_d(gt), "gt")
    if pred.dim() != 4 or pred.shape[-1] != 3 or pred.shape != gt.shape:
        raise ValueError("%s: pred and gt must both be [N, H, W, 3], got %s and %s" % (what, tuple(pred.shape), tuple(gt.shape)))
    if pred.device != gt.device:
        raise ValueError("%s: pred and gt are on different devices" % what)
    return pred, gt


def _metrics_ws(lib, n, h, w, device, what):
    nbytes = lib.shdr_metrics_workspace_bytes(n, h, w)
    if nbytes < 0:
        _lib.check(int(nbytes), what)
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64)


def pair_moments(pred, gt, normalise=True):
    """(scale_pred, scale_gt, peak), float64 [N]: the mean-normalisation scales 0.5 / (1e-6 + mean) of both images (1 without
    `normalise`) and the peak max(max(scale_gt * gt, 0)) of the ground truth"""
    lib = _lib.load()
    pred, gt = _pair(pred, gt, "pair_moments")
    n, h, w, _ = pred.shape
    ws = _metrics_ws(lib, n, h, w, pred.device, "shdr_pair_moments_f32")
    out = torch.empty((3, n), device=pred.device, dtype=torch.float64)
    _lib.check(lib.shdr_pair_moments_f32(_ptr(pred), _ptr(gt), n, h, w, int(bool(normalise)), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                         _ptr(ws), _stream()), "shdr_pair_moments_f32")
    return out[0], out[1], out[2]


def hdr_metrics(pred, gt, normalise=True, mu=5000.0):
    """Per-image quality of an HDR estimate, float64 device tensors [N] (definitions: include/shdr.h "validation metrics"):
    mse_l, mse_mu, l1_logc, ssim_mu, peak, scale_pred, scale_gt.  Two stream-ordered launches, no host synchronisation; the same
    inputs give the same bits.  An all-black gt (peak 0) gives the IEEE results (NaN / inf)."""
    lib = _lib.load()
    pred, gt = _pair(pred, gt, "hdr_metrics")
    n, h, w, _ = pred.shape
    ws = _metrics_ws(lib, n, h, w, pred.device, "shdr_hdr_metrics_f32")
    out = torch.empty((7, n), device=pred.device, dtype=torch.float64)
    sp, sg, peak = out[4], out[5], out[6]
    _lib.check(lib.shdr_pair_moments_f32(_ptr(pred), _ptr(gt), n, h, w, int(bool(normalise)), _ptr(sp), _ptr(sg), _ptr(peak), _ptr(ws),
                                         _stream()), "shdr_pair_moments_f32")
    _lib.check(lib.shdr_hdr_metrics_f32(_ptr(pred), _ptr(gt), n, h, w, float(mu), _ptr(sp), _ptr(sg), _ptr(peak), _ptr(out[0]),
                                        _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), _ptr(ws), _stream()), "shdr_hdr_metrics_f32")
    return dict(mse_l=out[0], mse_mu=out[1], l1_logc=out[2], ssim_mu=out[3], peak=peak, scale_pred=sp, scale_gt=sg)


def tonemap_u8(x, peak=None, reverse_channels=False, mu=5000.0):
    """float [N, H, W, 3] (or [H, W, 3]) -> uint8 of the same shape: round(255 * T(max(x, 0))^(1/2.2)) with the tone curve T of
    hdr_metrics.  peak: float64 device tensor with one value per image; None -> the image's maximum."""
    lib = _lib.load()
    x = _chk(_d(x), "x")
    shape = tuple(x.shape)
    x4 = x if x.dim() == 4 else x[None]
    if x4.dim() != 4 or x4.shape[-1] != 3:
        raise ValueError("tonemap_u8: expected [N, H, W, 3] or [H, W, 3], got %s" % (shape,))
    n, h, w, _ = x4.shape
    if peak is None:
        peak = pair_moments(x4, x4, normalise=False)[2]
    else:
        peak = _chk(peak, "peak", torch.float64).reshape(-1)
        if peak.numel() != n:
            raise ValueError("tonemap_u8: one peak per image")
    y = torch.empty(shape, device=x.device, dtype=torch.uint8)
    _lib.check(lib.shdr_tonemap_u8_f32(_ptr(x4), None, _ptr(peak), _ptr(y), n, h, w, float(mu), int(reverse_channels), _stream()),
               "shdr_tonemap_u8_f32")
    return y


# ---------------------------------------------------------------------------
# gain maps (ultrahdr.py), see csrc/gainmap.hip and csrc/gainmap.h
# ---------------------------------------------------------------------------
GAINMAP_FACTORS = (1, 2, 4, 8)
GAINMAP_STAGE_NAMES = ("statistics", "cells", "quantise")       # SHDR_GAINMAP_STAGES
GAINMAP_GUARD = 0xA5                                            # what the guard bytes of gainmap_encode / gainmap_apply(..., guard=) hold
GAINMAP_OFFSET = 0.015625                                       # OffsetSDR = OffsetHDR of every map written here
GAINMAP_IMAGE_DTYPE = np.dtype([("pix_off", np.int64), ("cell_off", np.int64), ("height", np.int32), ("width", np.int32),
                                ("factor", np.int32), ("stat_block0", np.int32), ("cell_block0", np.int32),
                                ("reserved", np.int32)])       # shdr_gainmap_image
GAINMAP_META_DTYPE = np.dtype([("gain_min", np.float32), ("gain_max", np.float32), ("scale", np.float32), ("reserved", np.int32),
                               ("count", np.int64)])            # shdr_gainmap_meta
GAINMAP_APPLY_DTYPE = np.dtype([("pix_off", np.int64), ("map_off", np.int64), ("height", np.int32), ("width", np.int32),
                                ("map_height", np.int32), ("map_width", np.int32), ("factor", np.int32), ("map_channels", np.int32),
                                ("gain_min", np.float32), ("gain_max", np.float32), ("gamma", np.float32), ("offset_sdr", np.float32),
                                ("offset_hdr", np.float32), ("weight", np.float32), ("block0", np.int32),
                                ("reserved", np.int32)])        # shdr_gainmap_apply_image
assert GAINMAP_IMAGE_DTYPE.itemsize == 40 and GAINMAP_META_DTYPE.itemsize == 24 and GAINMAP_APPLY_DTYPE.itemsize == 72


def _gainmap_fail(lib, rc):
    if rc != 0:
        raise ValueError(lib.shdr_last_error().decode())


def gainmap_math_host(op, x=None):
    """the polynomials and the table of csrc/gainmap.h on the host: op "log2" | "exp2" of a float32 array, or "srgb": the 256 entries"""
    lib = _lib.load()
    if op == "srgb":
        y = np.empty(256, dtype=np.float32)
        _gainmap_fail(lib, lib.shdr_gainmap_math_host(2, None, 256, _hptr(y)))
        return y
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    _gainmap_fail(lib, lib.shdr_gainmap_math_host({"log2": 0, "exp2": 1}[op], _hptr(x), x.size, _hptr(y)))
    return y


def gainmap_images(shapes, factor=4):
    """(descriptors GAINMAP_IMAGE_DTYPE [n], bytes of all maps, bytes of the workspace) of images of `shapes` [(H, W)] that lie back to
    back in the arenas; factor: one value or one per image.  ValueError for a shape or factor outside the scope."""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    factors = list(factor) if isinstance(factor, (list, tuple, np.ndarray)) else [factor] * len(shapes)
    if len(factors) != len(shapes):
        raise ValueError("gainmap_images: %d factors for %d images" % (len(factors), len(shapes)))
    images = np.zeros(len(shapes), dtype=GAINMAP_IMAGE_DTYPE)
    pix = 0
    for i, (shape, f) in enumerate(zip(shapes, factors)):
        if len(shape) != 2:
            raise ValueError("gainmap_images: image %d is %s: expected (H, W)" % (i, shape))
        images[i]["pix_off"], images[i]["height"], images[i]["width"], images[i]["factor"] = pix, shape[0], shape[1], int(f)
        pix += max(shape[0], 0) * max(shape[1], 0)
    return (images,) + gainmap_sizes(images)


def gainmap_sizes(images):
    """fills the derived fields of descriptors (in place); returns (bytes of all maps, bytes of the workspace)"""
    lib = _lib.load()
    if images.dtype != GAINMAP_IMAGE_DTYPE or images.ndim != 1 or not images.flags.c_contiguous:
        raise ValueError("gainmap_sizes: expected descriptors of GAINMAP_IMAGE_DTYPE")
    map_b, ws_b = ctypes.c_int64(0), ctypes.c_int64(0)
    _gainmap_fail(lib, lib.shdr_gainmap_encode_sizes(_hptr(images), images.size, ctypes.byref(map_b), ctypes.byref(ws_b)))
    return map_b.value, ws_b.value


def _gainmap_encode_args(what, images, scales, log2_range):
    images = np.ascontiguousarray(images)
    if images.dtype != GAINMAP_IMAGE_DTYPE or images.ndim != 1:
        raise ValueError("%s: expected descriptors of GAINMAP_IMAGE_DTYPE (gainmap_images)" % what)
    if scales is not None:
        scales = np.ascontiguousarray(scales, dtype=np.float32).reshape(-1)
        if scales.size != images.size:
            raise ValueError("%s: %d scales for %d images" % (what, scales.size, images.size))
    lo, hi = (float(v) for v in log2_range)
    return images, scales, lo, hi


def gainmap_encode_host(sdr, hdr, images, scales=None, log2_range=(-4.0, 8.0), reverse_channels=False, map_capacity=None, meta_capacity=None):
    """the host twin of gainmap_encode: sdr uint8 / hdr float32 host arenas [arena_pixels, 3] -> (maps uint8 [map bytes], meta
    GAINMAP_META_DTYPE [n]).  map_capacity, meta_capacity: the sizes of the destinations (default: what is needed); a smaller one
    raises ValueError and nothing is written."""
    lib = _lib.load()
    images, scales, lo, hi = _gainmap_encode_args("gainmap_encode_host", images, scales, log2_range)
    sdr, hdr = np.ascontiguousarray(sdr), np.ascontiguousarray(hdr)
    if sdr.dtype != np.uint8 or hdr.dtype != np.float32 or sdr.size != hdr.size or sdr.size % 3:
        raise ValueError("gainmap_encode_host: the arenas must hold the same pixels, uint8 and float32 [arena_pixels, 3]")
    need = int(sum(3 * (-(-int(im["height"]) // max(int(im["factor"]), 1))) * (-(-int(im["width"]) // max(int(im["factor"]), 1))) for im in images))
    map_cap = need if map_capacity is None else int(map_capacity)
    meta_cap = images.size if meta_capacity is None else int(meta_capacity)
    maps = np.full(max(map_cap, 1), GAINMAP_GUARD, dtype=np.uint8)
    meta = np.zeros(max(meta_cap, 1), dtype=GAINMAP_META_DTYPE)
    _gainmap_fail(lib, lib.shdr_gainmap_encode_host(_hptr(sdr), _hptr(hdr), sdr.size // 3, _hptr(images), images.size,
                                                   None if scales is None else _hptr(scales), lo, hi, int(bool(reverse_channels)),
                                                   _hptr(maps), map_cap, _hptr(meta), meta_cap))
    return maps[:need], meta[:images.size]


def _guarded(size, guard, dev):
    """(raw, inner): `size` bytes with `guard` bytes of GAINMAP_GUARD on both sides (a multiple of 16: the inner part stays aligned)"""
    if not guard:
        raw = torch.empty(max(size, 1), device=dev, dtype=torch.uint8)
        return raw, raw[:size]
    raw = torch.full((size + 2 * guard,), GAINMAP_GUARD, device=dev, dtype=torch.uint8)
    return raw, raw[guard:guard + size]


def gainmap_encode(sdr, hdr, images, scales=None, log2_range=(-4.0, 8.0), reverse_channels=False, stage_ms=None, guard=0, info=None):
    """Gain maps of a batch of SDR / HDR pairs on the device (csrc/gainmap.hip): bit for bit what gainmap_encode_host computes.
    sdr uint8 / hdr float32 device arenas [arena_pixels, 3] (flat), images: descriptors (gainmap_images), scales: one fixed exposure
    scale per image, or None for the alignment of include/shdr.h.  Returns (maps uint8 [map bytes], meta uint8 [24 n]: the records of
    GAINMAP_META_DTYPE) on the device; image i's map starts at byte 3 images[i]["cell_off"].  Three stream-ordered launches, no host
    wait.  stage_ms: receives the device times of GAINMAP_STAGE_NAMES; guard: bytes of GAINMAP_GUARD around maps, meta and
    workspace, returned through `info` (a dict).  A descriptor that libshdr refuses raises ValueError before anything is launched."""
    lib = _lib.load()
    sdr, hdr = _chk(sdr, "sdr", torch.uint8), _chk(hdr, "hdr")
    if sdr.numel() != hdr.numel() or sdr.numel() % 3 or sdr.device != hdr.device:
        raise ValueError("gainmap_encode: the arenas must hold the same pixels, uint8 and float32 [arena_pixels, 3], on one device")
    images, scales, lo, hi = _gainmap_encode_args("gainmap_encode", images, scales, log2_range)
    dev = sdr.device
    derived = images.copy()
    map_b, ws_b = gainmap_sizes(derived)                           # refuses shapes and factors; the derived fields are checked by the call
    guard = (int(guard) + 15) // 16 * 16
    maps_raw, maps = _guarded(map_b, guard, dev)
    meta_raw, meta = _guarded(24 * images.size, guard, dev)
    ws_raw, ws = _guarded(ws_b, guard, dev)
    images_dev = torch.from_numpy(images.view(np.uint8).copy()).to(dev)
    scales_dev = None if scales is None else torch.from_numpy(scales).to(dev)
    with _stage_times(stage_ms, len(GAINMAP_STAGE_NAMES)) as ms:
        _gainmap_fail(lib, lib.shdr_gainmap_encode(_ptr(sdr), _ptr(hdr), sdr.numel() // 3, _hptr(images), _ptr(images_dev), images.size,
                                                  None if scales is None else _hptr(scales), _ptr(scales_dev), lo, hi,
                                                  int(bool(reverse_channels)), _ptr(maps), map_b, _ptr(meta), images.size, _ptr(ws),
                                                  _stream(), ms))
    if info is not None:
        info.update(maps_raw=maps_raw, meta_raw=meta_raw, workspace_raw=ws_raw, guard=guard, map_bytes=map_b, workspace_bytes=ws_b)
    return maps, meta


def gainmap_apply_images(items):
    """descriptors GAINMAP_APPLY_DTYPE [n] of images whose SDR pixels and maps lie back to back.  items: dicts with height, width, factor,
    map_channels, gain_min, gain_max and optionally gamma (1), offset_sdr, offset_hdr (1 / 64), weight (1).  Returns (descriptors,
    blocks of the launch); ValueError for what libshdr refuses."""
    lib = _lib.load()
    images = np.zeros(len(items), dtype=GAINMAP_APPLY_DTYPE)
    pix = off = 0
    for i, it in enumerate(items):
        h, w, f, mc = (int(it[k]) for k in ("height", "width", "factor", "map_channels"))
        mh, mw = -(-h // max(f, 1)), -(-w // max(f, 1))
        images[i] = (pix, off, h, w, mh, mw, f, mc, it["gain_min"], it["gain_max"], it.get("gamma", 1.0), it.get("offset_sdr", GAINMAP_OFFSET),
                     it.get("offset_hdr", GAINMAP_OFFSET), it.get("weight", 1.0), 0, 0)
        pix += max(h, 0) * max(w, 0)
        off += max(mh * mw * mc, 0)
    blocks = ctypes.c_int64(0)
    _gainmap_fail(lib, lib.shdr_gainmap_apply_sizes(_hptr(images), images.size, ctypes.byref(blocks)))
    return images, blocks.value


def _gainmap_apply_args(what, images):
    images = np.ascontiguousarray(images)
    if images.dtype != GAINMAP_APPLY_DTYPE or images.ndim != 1:
        raise ValueError("%s: expected descriptors of GAINMAP_APPLY_DTYPE (gainmap_apply_images)" % what)
    return images


def gainmap_apply_host(sdr, maps, images, out_capacity=None):
    """the host twin of gainmap_apply: sdr uint8 [arena_pixels, 3], maps uint8 (flat) -> float32 [arena_pixels, 3]; out_capacity: the
    destination's size in pixels (default: the arena's)"""
    lib = _lib.load()
    images = _gainmap_apply_args("gainmap_apply_host", images)
    sdr, maps = np.ascontiguousarray(sdr), np.ascontiguousarray(maps)
    if sdr.dtype != np.uint8 or maps.dtype != np.uint8 or sdr.size % 3:
        raise ValueError("gainmap_apply_host: expected uint8 pixels [arena_pixels, 3] and uint8 maps")
    cap = sdr.size // 3 if out_capacity is None else int(out_capacity)
    out = np.zeros((max(cap, 1), 3), dtype=np.float32)
    _gainmap_fail(lib, lib.shdr_gainmap_apply_host(_hptr(sdr), sdr.size // 3, _hptr(maps), maps.size, _hptr(images), images.size, _hptr(out), cap))
    return out[:cap]


def gainmap_apply(sdr, maps, images, guard=0, info=None):
    """HDR pixels of a batch of SDR images and their gain maps, one launch (csrc/gainmap.hip): bit for bit gainmap_apply_host.  sdr
    uint8 device arena [arena_pixels, 3], maps uint8 device bytes, images: descriptors (gainmap_apply_images).  Returns float32
    [arena_pixels, 3] on the device.  guard: bytes of GAINMAP_GUARD around the output, returned through `info`."""
    lib = _lib.load()
    images = _gainmap_apply_args("gainmap_apply", images)
    sdr, maps = _chk(sdr, "sdr", torch.uint8), _chk(maps, "maps", torch.uint8)
    if sdr.numel() % 3 or sdr.device != maps.device:
        raise ValueError("gainmap_apply: expected uint8 pixels [arena_pixels, 3] and the maps on one device")
    pixels = sdr.numel() // 3
    guard = (int(guard) + 15) // 16 * 16
    out_raw, out = _guarded(12 * pixels, guard, sdr.device)
    images_dev = torch.from_numpy(images.view(np.uint8).copy()).to(sdr.device)
    _gainmap_fail(lib, lib.shdr_gainmap_apply(_ptr(sdr), pixels, _ptr(maps), maps.numel(), _hptr(images), _ptr(images_dev), images.size,
                                             _ptr(out), pixels, _stream()))
    if info is not None:
        info.update(out_raw=out_raw, guard=guard)
    return out.view(torch.float32).view(pixels, 3)
