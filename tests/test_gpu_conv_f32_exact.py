"""The exact-fp32 convolution kernels -- conv_mfma_dma_kernel, conv_mfma_kernel, conv_rega_kernel, conv_direct_kernel (csrc/conv.hip),
winograd_fused_kernel<R, UP> (csrc/winograd_fused.hip), the four transform kernels of the "planes" plan (csrc/winograd.hip) and the
input-gradient plumbing of csrc/conv_plan.hip (dgrad_filter_kernel, subfilter_kernel, the polyphase stride-2 form, strided output
placement) -- against the float64 statement of tests/conv_ref.py, EXACTLY and element by element.

Exactness comes from the operands, not from a tolerance.  Three operand modes, one fixed seed per case id:
  int     x integers in [-2, 2], w in {-1, 0, 1}: layout, taps, chunks, edges;
  fx      x = (k + j 2^-11) 2^-7 with integer w: the activations need more than 11 mantissa bits;
  fw      integer x with w = q / 2 + r 2^-13: the filter does.
(Never both: the products would need 2^-22 resolution.)  A kernel that ran an operand through fp16, bf16 or a truncated format would
differ in a fine mode.  Every case asserts on the reference, BEFORE the kernel is called, that the sum of absolute terms of every
output is below 2^24 units of the terms' common lsb: an fp32 accumulator then holds every partial sum exactly, in any order (MFMA
order, chunks, taps, FMA chains).  The Winograd cases assert the same bound in the transform domain (conv_ref.winograd_conv: per
transform position the channel sum of |B^T d B| |G g G^T|, and the 16-term output transform): F(2x2, 3x3) only adds and halves, every
intermediate is a multiple of a small power of two, and the kernels must reproduce the direct convolution bit for bit.  The epilogue
is conv_ref.epilogue: one fp32 rounding per step; biases, shifts and residuals are integers, scales powers of two.  The PREC 1 / 2
forms (fp16 / bf16 MFMA operands) are held to the model that rounds both operands to nearest-even and then convolves exactly.

Every comparison is whole-tensor equality of bit patterns with -0 mapped to +0; a difference names the first differing index, its
tile and got / want.  Every output and range slot sits between guard words of a NaN pattern; the gaps of a strided or padded output
must keep that pattern.  The slot must hold the bits of max |y_ref| (or a larger value it held before).  The C ABI is called through
shdr._lib.  tests/test_conv_ref.py checks every precondition on the CPU and proves that the inputs are not degenerate (a dropped tap,
a shifted pad, a dropped k-chunk, swapped sources, a zeroed halo column, a shifted phase or fp16 operands each change an output).

Which instantiation a case runs is DERIVED FROM THE DISPATCH CODE (shdr_conv2d_fwd_yrange_f32 / launch_mfma / rega_ok / dispatch_rega in
conv.hip, plan_of / dgrad_geom in conv_plan.hip), restated in `instance()`; the plan is asked from the library and asserted where a
plan exists.  The plans are forced with the existing switches and algo values only.

instantiation -> cases (T = test_mfma_tile_forms, ids "<kernel>_<tile>_..."; the same configurations run on both staging kernels):
  conv_mfma_dma_kernel<128,128,2,2, FAST | !FAST>     T dma_t128_*                     (K > 128: 5 .. 18 chunks)
  conv_mfma_dma_kernel<128,64,4,1, FAST | !FAST>      T dma_t64_* (incl. the 1x1 K = 128 -> 128 couts case), epilogue_dma64_*, legacy_*
  conv_mfma_dma_kernel<128,32,4,1, FAST | !FAST>      T dma_t32_*, geo_dma_*, out_dma32_*, epilogue_dma32_*, rega_refused_*
  conv_mfma_dma_kernel<128,16,4,1, FAST | !FAST>      T dma_t16_*, out_dma16_*, epilogue_dma16_*, wbs_*
  conv_mfma_kernel<the four tiles, FAST | !FAST>      T reg_t*_ (SHDR_ALGO_MFMA_REG), x2s_t*_ (x2_scale = 2^-k), geo_reg_*, out_reg_*, epilogue_reg_*
  conv_mfma_dma_kernel<.., PREC 1 | 2>                prec_* (SHDR_ALGO_MFMA_F16 / _BF16 / AUTO_F16 / AUTO_BF16)
  conv_rega_kernel<4, NT 1|2, CT 4|16|32, KK 0|3|5|7> rega_* (KK 0: rega_k1x3_*, rega_nodpp_*), rega_persistent_*, prec_auto_*_rega_*
  conv_rega_kernel<4, 4, 4, 3>                        rega_image64_*
  conv_direct_kernel<3 | 8 | 16>                      direct_*
  winograd_fused_kernel<1>, <2>, <1, true>            wf_*, wf16_* (SHDR_WINOGRAD_TILE=16), wfup_*, dgrad_wino_*
  winograd_{filter, filter_packed, input, output}     test_winograd_transform_kernels, planes_* (+ the 16-"image" 1x1 GEMM with w_batch_stride)
  dgrad_filter_kernel, subfilter_kernel, pad_channels dgrad_* (stride 1 MFMA / Winograd, 1x1 / 2, polyphase 3x3 / 2 and 7x7 / 2)
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as C
from test_gpu_conv_x3_exact import EPILOGUES, PLAN, K, Slot, dev, epilogue_operands, fine_w, fine_x, int_w, int_x, lib, same, seed_of  # noqa: F401 (K, lib: fixtures)
from test_gpu_wgrad_f32_exact import GUARD, SENT32, P, guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

LIMIT = 2.0 ** 24
E_SHAPE, E_ALIGN, E_NULL = -1, -2, -5
ALGO = dict(auto=0, mfma=1, direct=2, reg=3, f16=4, bf16=5, auto_f16=6, auto_bf16=7, exact=8)
S4 = 2.0 ** -4


# ---------------------------------------------------------------------------------------------------------------------------------
# cases, operands, the model (pure NumPy: tests/test_conv_ref.py runs all of it on the CPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def fc(name, algo, n, h, w, c1, c2, cout, k, stride=1, mode="int", epi="plain", **o):
    kh, kw = (k, k) if isinstance(k, int) else k
    o.update(name=name, algo=algo, n=n, h=h, w=w, c1=c1, c2=c2, cout=cout, kh=kh, kw=kw, stride=stride, mode=mode, epi=epi)
    o.setdefault("env", {})
    o.setdefault("x2s", 1.0)
    return pytest.param(o, id=name)


def geometry(o):
    """(Ho, Wo, pad_t, pad_l) of a case: TF 'SAME' unless `pad` / `out` replace it"""
    ho, pt = C.same_pad(o["h"], o["kh"], o["stride"])
    wo, pl = C.same_pad(o["w"], o["kw"], o["stride"])
    if o.get("pad") is not None:
        pt, pl = o["pad"]
    if o.get("out") is not None:
        ho, wo = o["out"]
    return ho, wo, pt, pl


def operands(o):
    """(x, x2, w): the second source holds integers times 1 / x2_scale (a power of two) -- next to a fine first source m 2^-8 / x2_scale,
    so that both sources' terms share a small lsb.  `wbs`: one filter per image, [N, KH, KW, Ct, Cout]."""
    rng = np.random.default_rng(seed_of(o["name"]))
    n, h, w, c1, c2, cout = (o[f] for f in ("n", "h", "w", "c1", "c2", "cout"))
    keep, fine = o.get("keep", 1.0), o["mode"] == "fx"
    x = fine_x(rng, (n, h, w, c1), keep, o.get("kmax", 2))[0] if fine else int_x(rng, (n, h, w, c1), keep)[0]
    x2 = None
    if c2:
        x2 = int_x(rng, (n, h, w, c2), keep)[0]
        x2 = (np.ldexp(x2, -8) if fine else x2) / o["x2s"]
    shape = (o["kh"], o["kw"], c1 + c2, cout)
    cv = o.get("cv") or cout
    one = lambda: fine_w(rng, shape, keep, cv if cv != cout else None)[0] if o["mode"] == "fw" else int_w(rng, shape, keep, cv if cv != cout else None)
    wt = np.stack([one() for _ in range(n)]) if o.get("wbs") else one()
    return x, x2, wt


def rounded(a, prec):
    if a is None or not prec:
        return a
    return C.to_f16(a).astype(np.float64) if prec == 1 else C.to_bf16(a)


def chunk_rows(o):
    """the k rows (tap-major, channel-minor: the HWIO order) of the LAST 32-wide k-chunk of the implicit GEMM"""
    kk = o["kh"] * o["kw"] * (o["c1"] + o["c2"])
    return kk - ((kk - 1) % 32 + 1), kk


def model(o, x, x2, wt, wrong=None, probe=False):
    """(z, sum |terms|, lsb) in float64.  `wrong` names a deliberately wrong model for the sensitivity check of tests/test_conv_ref.py;
    `probe` replaces every operand by ones (times 1 / x2_scale): whether a wrong model CAN show in the geometry of the case."""
    ho, wo, pt, pl = geometry(o)
    if probe:
        x, x2, wt = np.ones_like(x), None if x2 is None else np.ones_like(x2) / o["x2s"], np.ones_like(wt)
    c1, c2, x2s, prec = o["c1"], o["c2"], o["x2s"], precision(o)
    if wrong == "f16":                                                      # operands through fp16 where the kernel keeps fp32 (and back)
        prec = 1 if prec == 0 else 0
    x, x2, wt = rounded(x, prec), rounded(x2, prec), rounded(wt, prec)
    if wrong == "tap":
        wt = wt.copy()
        wt[..., min(pt, o["kh"] - 1), min(pl, o["kw"] - 1), :, :] = 0.0          # the tap that reads x[0, 0] for y[0, 0]: inside every image
    if wrong == "pad":
        pl = pl - 1 if pl > 0 else pl + 1
    if wrong == "chunk":
        a, b = chunk_rows(o)
        wt = wt.copy().reshape(wt.shape[:-4] + (b, o["cout"]))
        wt[..., a:b, :] = 0.0
        wt = wt.reshape(wt.shape[:-2] + (o["kh"], o["kw"], c1 + c2, o["cout"]))
    if wrong == "swap":
        wt = np.roll(wt, -c2, axis=-2)                                      # concat[x2, x] instead of concat[x, x2]
    if wrong == "halo":
        x = x.copy()
        x[:, :, min(16, o["w"] - 1)] = 0.0                                  # the column right of the first 16-column tile (iw0 + 16)
        if x2 is not None:
            x2 = x2.copy()
            x2[:, :, min(16, o["w"] - 1)] = 0.0
    kw = dict(stride=o["stride"], pad=(pt, pl), out_hw=(ho, wo))
    conv = lambda a, a2, f, s: (np.concatenate([C.conv2d(a[i:i + 1], None if a2 is None else a2[i:i + 1], f[i], None, x2_scale=s, **kw)
                                                for i in range(o["n"])]) if o.get("wbs") else C.conv2d(a, a2, f, None, x2_scale=s, **kw))
    z = conv(x, x2, wt, x2s)
    total = conv(np.abs(x), None if x2 is None else np.abs(x2), np.abs(wt), abs(x2s))
    lsb = C.common_lsb(x) * C.common_lsb(wt[..., :c1, :])
    if c2:
        lsb = min(lsb, C.common_lsb(x2 * x2s) * C.common_lsb(wt[..., c1:, :]))
    return z, total, lsb


def precision(o):
    """a.prec of shdr_conv2d_fwd_yrange_f32 BEFORE the register-A hand-back: 1 fp16 / 2 bf16 MFMA operands, 0 exact"""
    algo = o["algo"]
    if algo in ("f16", "bf16"):
        return 1 if algo == "f16" else 2
    if algo in ("auto_f16", "auto_bf16") and mfma_ok(o) and o["x2s"] == 1.0 and not rega(o):
        return 1 if algo == "auto_f16" else 2
    return 0


def mfma_ok(o):
    cv = o.get("cv") or o["cout"]
    ycs = o.get("ycs") or cv
    rcs = cv + o.get("res_pad", 8)
    dense = cv % 4 != 0 or (ycs % 4 == 0 and (o["epi"] != "res" or rcs % 4 == 0))
    return o["c1"] % 4 == 0 and o["c2"] % 4 == 0 and o["cout"] % 16 == 0 and dense and not o.get("lead")


def rega_ok(o):
    """rega_ok of conv.hip: narrow stride-1 layers, 4 / 16 / 32 channels per tap, the filter in at most 100 KB of LDS"""
    c1, c2, cout, kh, kw = o["c1"], o["c2"], o["cout"], o["kh"], o["kw"]
    if o["stride"] != 1 or o.get("wbs") or cout % 16:
        return False
    if cout > 32 and not (cout == 64 and c2 == 0 and c1 == 4 and (kh, kw) == (3, 3) and "SHDR_NO_REGA64" not in o["env"]):
        return False
    if not ((c2 == 0 and c1 in (4, 8, 12, 16)) or (c1 == 16 and c2 == 16)):
        return False
    return kh * kw * (c1 + c2) * cout * 4 <= 100 * 1024


def rega(o):
    algo = o["algo"]
    if algo not in ("auto", "exact", "auto_f16", "auto_bf16") or not mfma_ok(o) or "SHDR_NO_REGA" in o["env"]:
        return False
    if o["cout"] % 128 == 0 and o["kh"] * o["kw"] * (o["c1"] + o["c2"]) > 128:
        return False
    reduced = algo in ("auto_f16", "auto_bf16") and o["x2s"] == 1.0
    return (not reduced or (o["c2"] == 0 and o["cout"] in (16, 64))) and rega_ok(o)


def instance(o):
    """the kernel instantiation shdr_conv2d_fwd_yrange_f32 launches for a case (see the module docstring); it labels the failure
    messages and is what the case lists are built from"""
    algo, c1, c2, cout, kh, kw = o["algo"], o["c1"], o["c2"], o["cout"], o["kh"], o["kw"]
    ct, kk = c1 + c2, kh * kw * (c1 + c2)
    if algo == "direct" or (algo in ("auto", "exact", "auto_f16", "auto_bf16") and not mfma_ok(o)):
        return "conv_direct_kernel<%d>" % (3 if cout <= 3 else (16 if cout % 16 == 0 else 8))
    if cout % 128 == 0 and kk > 128:
        tile = "128, 128, 2, 2"
    elif rega(o):
        if cout == 64:
            return "conv_rega_kernel<4, 4, 4, 3>"
        dpp = kh == kw and kh in (3, 5, 7) and "SHDR_REGA_NO_DPP" not in o["env"]
        return "conv_rega_kernel<4, %d, %d, %d>" % (cout // 16, 4 if ct == 4 else (16 if ct <= 16 else 32), kh if dpp else 0)
    else:
        tile = "128, 64, 4, 1" if cout % 64 == 0 else ("128, 32, 4, 1" if cout % 32 == 0 else "128, 16, 4, 1")
    fast = "true" if ct % 32 == 0 and (c2 == 0 or c1 % 32 == 0) else "false"
    prec = precision(o)
    if prec or (o["x2s"] == 1.0 and algo != "reg"):
        return "conv_mfma_dma_kernel<%s, %s%s>" % (tile, fast, ", %d" % prec if prec else "")
    return "conv_mfma_kernel<%s, %s>" % (tile, fast)


def tile_of(o):
    name = instance(o)
    return (16, 16) if "rega" in name else ((8, 16) if "mfma" in name else (1, 256))


def reference(o, wrong=None, probe=False):
    """everything of a case that needs no device: operands, the model, the precondition, the expected output"""
    name, cout = o["name"], o["cout"]
    cv = o.get("cv") or cout
    x, x2, wt = operands(o)
    ho, wo, pt, pl = geometry(o)
    z, total, lsb = model(o, x, x2, wt, wrong, probe)
    if probe:
        return dict(y=z[..., :cv])
    worst = float(total.max()) / lsb
    assert worst < LIMIT, "%s: sum |terms| / lsb = %.3g 2^24: the accumulator is not exact by construction" % (name, worst / LIMIT)
    bias, act1, scale, shift, res, act2 = epilogue_operands(name, o["epi"], cv, (o["n"], ho, wo), o.get("res_pad", 8))
    z = z[..., :cv]
    if bias is not None:
        z = z + bias
    y = C.epilogue(z, act1, scale, shift, res, act2)
    return dict(x=x, x2=x2, w=wt, bias=bias, act1=act1, scale=scale, shift=shift, res=res, act2=act2, y=y, cv=cv, ho=ho, wo=wo, pt=pt, pl=pl,
                ymax=float(np.abs(y).max()), worst=worst / LIMIT)


def wrong_models(o):
    """the deliberately wrong models that apply to a forward case"""
    names = ["tap", "pad", "chunk", "halo"]
    if o["c2"]:
        names.append("swap")
    if o["mode"] != "int":
        names.append("f16")
    return names


def plan_expected(o):
    """plan_of of conv_plan.hip for the algo values used here (AUTO_EXACT never plans the split-operand kernels)"""
    if o["algo"] != "exact":
        return "direct" if o["algo"] == "direct" else "mfma"
    ho, wo, pt, pl = geometry(o)
    cv = o.get("cv") or o["cout"]
    ct = o["c1"] + o["c2"]
    same_geo = (ho, pt) == C.same_pad(o["h"], o["kh"], o["stride"]) and (wo, pl) == C.same_pad(o["w"], o["kw"], o["stride"])
    if ((o["kh"], o["kw"], o["stride"]) == (3, 3, 1) and same_geo and o["epi"] != "res" and cv == o["cout"] and not o.get("wbs") and not o.get("ypix")
            and "SHDR_NO_WINOGRAD" not in o["env"]):
        two_ok = o["c2"] == 0 or (o["c2"] == o["c1"] and o["c1"] % 8 == 0 and o["x2s"] == 1.0)
        if two_ok and ct % 8 == 0 and o["cout"] % 64 == 0 and ct >= 32:
            return "fused"
        if o["c2"] == 0 and ct % 32 == 0 and o["cout"] % 16 == 0 and min(ct, o["cout"]) >= 128 and ct * o["cout"] >= 32768:
            return "planes"
    return "mfma" if o["c1"] % 4 == 0 and o["c2"] % 4 == 0 and o["cout"] % 16 == 0 else "direct"


# ---------------------------------------------------------------------------------------------------------------------------------
# device helpers
# ---------------------------------------------------------------------------------------------------------------------------------
class Out:
    """an output tensor between guard words; `lead` words into the 16-byte aligned view (an unaligned pointer)"""

    def __init__(self, shape, lead=0):
        self.shape, self.numel, self.lead = tuple(shape), int(np.prod(shape)), lead
        self.buf, view = guarded(self.numel + lead)
        self.ptr = ctypes.c_void_p(view.data_ptr() + 4 * lead)

    def words(self, what):
        guards_intact(self.buf, self.numel + self.lead, what)
        raw = self.buf.cpu().numpy().view(np.uint32)
        assert (raw[GUARD:GUARD + self.lead] == SENT32).all(), what + ": words BEFORE the tensor were written"
        return raw[GUARD + self.lead:GUARD + self.lead + self.numel].reshape(self.shape)


def dev_lead(a, lead=0):
    """(tensor that owns the memory, pointer to the operand `lead` words into it)"""
    if a is None:
        return None, None
    t = dev(a)
    if lead:
        buf = torch.zeros(t.numel() + 4, device="cuda")
        buf[lead:lead + t.numel()] = t.reshape(-1)
        return buf, P(buf, 4 * lead)
    return t, P(t)


def same_in_tiles(got, want, what, tile):
    """X.same, the message extended by the tile of THIS kernel (8 x 16 for the MFMA tiles, 16 x 16 for the register-A kernel)"""
    try:
        same(got, want, what)
    except AssertionError as e:
        bad = (np.asarray(got, dtype=np.float32) + np.float32(0)).view(np.uint32) != (np.asarray(want, dtype=np.float32) + np.float32(0)).view(np.uint32)
        i = np.unravel_index(int(np.argmax(bad)), bad.shape) if bad.shape == np.shape(want) and bad.any() else None
        where = "" if i is None or len(i) != 4 else " [tile (%d, %d) of %d x %d pixels]" % (i[1] // tile[0], i[2] // tile[1], tile[0], tile[1])
        raise AssertionError(str(e) + where) from None


def placed(words, o, r, what, tile):
    """compare the stored elements of a (possibly strided, channel-padded) output with y_ref; every other word keeps the guard pattern"""
    s, (oh, ow) = o.get("ypix", (1, (0, 0)))
    sub = words[:, oh::s, ow::s][:, :r["ho"], :r["wo"], :r["cv"]]
    same_in_tiles(np.ascontiguousarray(sub).view(np.float32), r["y"], what, tile)
    rest = words.copy()
    rest[:, oh::s, ow::s][:, :r["ho"], :r["wo"], :r["cv"]] = SENT32
    assert (rest == SENT32).all(), "%s: %d words in the gaps of y (between pixels / beyond cout_valid) were written" % (what, int((rest != SENT32).sum()))


def descriptor(K, o, r):
    d = K._conv_desc((o["n"], o["h"], o["w"], o["c1"]), (o["kh"], o["kw"], o["c1"] + o["c2"], o["cout"]), o["stride"], o["c2"], o["x2s"], r["cv"])
    d.pad_t, d.pad_l, d.Ho, d.Wo = r["pt"], r["pl"], r["ho"], r["wo"]
    d.act1, d.act2, d.algo = r["act1"], r["act2"], ALGO[o["algo"]]
    d.y_cstride = o.get("ycs") or 0
    d.res_cstride = 0 if r["res"] is None else r["res"].shape[3]
    if o.get("wbs"):
        d.w_batch_stride = o["kh"] * o["kw"] * (o["c1"] + o["c2"]) * o["cout"]
    if o.get("ypix"):
        d.y_pix_stride, (d.y_off_h, d.y_off_w) = o["ypix"]
        d.y_H, d.y_W = y_extent(o, r)
    return d


def y_extent(o, r):
    s = o.get("ypix", (1, (0, 0)))[0]
    return (r["ho"], r["wo"]) if s == 1 else (s * r["ho"] + 1, s * r["wo"] + 1)        # (one row / column more than the phases fill)


def run_forward(K, lib, o, monkeypatch, r=None, preset=None):
    """one call of shdr_conv2d_fwd_yrange_f32; y and the range slot between guards"""
    for name, value in o["env"].items():
        monkeypatch.setenv(name, value)
    r = r or reference(o)
    name = o["name"]
    d = descriptor(K, o, r)
    plan = PLAN[int(lib.shdr_conv2d_plan_f32(ctypes.byref(d), int(r["res"] is not None)))]
    assert plan == plan_expected(o), "%s: planned %s, expected %s" % (name, plan, plan_expected(o))
    what = "%s [%s]" % (name, instance(o))
    lead = o.get("lead", 0)
    keep = []                                                             # (the tensors that own the operands' memory)

    def arg(a):
        t, p = dev_lead(a, lead)
        keep.append(t)
        return p
    yh, yw = y_extent(o, r)
    ycs = o.get("ycs") or r["cv"]
    res = r["res"]
    if res is not None and o.get("ypix"):                                 # the residual is read where y is written
        s, (oh, ow) = o["ypix"]
        full = np.zeros((o["n"], yh, yw, res.shape[3]))
        full[:, oh::s, ow::s][:, :r["ho"], :r["wo"]] = res
        res = full
    out = Out((o["n"], yh, yw, ycs), lead)
    tracked = o.get("slot", True)
    slot = Slot((seed_of(name) % 4 == 0) * 1.0e6 if preset is None else preset) if tracked else None
    rc = lib.shdr_conv2d_fwd_yrange_f32(ctypes.byref(d), arg(r["x"]), arg(r["x2"]), arg(r["w"]), arg(r["bias"]), arg(r["scale"]), arg(r["shift"]),
                                        arg(res), out.ptr, P(slot.view) if tracked else None, K._stream())
    assert rc == 0, (what, rc, lib.shdr_last_error())
    placed(out.words(what + " y"), o, r, what + " y", tile_of(o))
    if tracked:
        slot.check(r["ymax"], what)


# ---------------------------------------------------------------------------------------------------------------------------------
# the tile forms of conv_mfma_dma_kernel and of its register-staged twin conv_mfma_kernel: <128,128,2,2>, <128,64,4,1>, <128,32,4,1>,
# <128,16,4,1>, each FAST (Ct % 32 == 0, sources split on a 32 boundary) and not; 1, 2, an odd and an even >= 4 number of k-chunks; the
# last chunk ragged and straddling taps (K % 32 != 0).  SHDR_ALGO_MFMA keeps the register-A kernel out of the way.
# ---------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 9), (8, 16), (9, 8), (15, 17), (16, 15), (17, 33), (33, 7), (16, 16), (1, 33), (33, 1), (15, 15)]   # from {1,7,8,9,15,16,17,33}^2
MODES = ("int", "fx", "fw")
# (C1, C2, kh, kw): chunks
FAST = [(32, 0, 1, 1), (64, 0, 1, 1), (32, 0, 3, 3), (32, 32, 1, 3)]                                  # 1, 2, 9, 6
SLOW = [(4, 0, 1, 1), (4, 0, 3, 3), (12, 0, 3, 3), (36, 0, 1, 3), (36, 0, 3, 3), (16, 16, 1, 1), (16, 16, 3, 3)]   # 1, 2, 4, 4, 11, 1, 9 (ragged but 16 + 16)
FAST128 = [(160, 0, 1, 1), (256, 0, 1, 1), (32, 0, 3, 3), (32, 32, 1, 3)]                             # 5, 8, 9, 6           (K > 128)
SLOW128 = [(4, 0, 7, 7), (12, 0, 5, 5), (36, 0, 3, 3), (16, 16, 3, 3)]                                # 7, 10, 11, 9
TILES = [("t128", 128, FAST128 + SLOW128), ("t64", 64, FAST + SLOW), ("t32", 32, FAST + SLOW), ("t16", 16, FAST + SLOW), ("t16", 48, FAST[:2] + SLOW[:2])]


def tile_cases():
    cases, i = [], 0
    for kernel, algo in (("dma", "mfma"), ("reg", "reg"), ("x2s", "mfma")):
        for tag, cout, configs in TILES:
            for c1, c2, kh, kw in configs:
                if kernel == "x2s" and not c2:
                    continue
                i += 1
                (h, w), n = SIZES[i % len(SIZES)], 1 + i % 2
                mode, epi = MODES[i % 3], EPILOGUES[i % len(EPILOGUES)]
                x2s = (S4 if i % 2 else 0.5) if kernel == "x2s" else 1.0
                name = "%s_%s_%d_%d_%d_k%dx%d_%dx%dx%d_%s_%s" % (kernel, tag, c1, c2, cout, kh, kw, n, h, w, mode, epi)
                cases.append(fc(name, algo, n, h, w, c1, c2, cout, (kh, kw), mode=mode, epi=epi, x2s=x2s))
    # the 1x1 layer with K = 128 and 128 couts lands on the 64-cout tile (K > 128 is the rule of the 128-cout tile)
    cases.append(fc("dma_t64_128_0_128_k1x1_2x15x17_fx_relu", "mfma", 2, 15, 17, 128, 0, 128, 1, mode="fx", epi="relu"))
    cases.append(fc("reg_t64_128_0_128_k1x1_1x17x33_fw_res", "reg", 1, 17, 33, 128, 0, 128, 1, mode="fw", epi="res"))
    return cases


TILE_CASES = tile_cases()


@pytest.mark.parametrize("o", TILE_CASES)
def test_mfma_tile_forms(K, lib, o, monkeypatch):
    name = instance(o)
    assert ("conv_mfma_dma_kernel" if o["name"].startswith("dma") else "conv_mfma_kernel<") in name, name
    tag = o["name"].split("_")[1]
    assert {"t128": "<128, 128", "t64": "<128, 64", "t32": "<128, 32", "t16": "<128, 16"}[tag] in name, name
    run_forward(K, lib, o, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry on both staging kernels: k 1 / 3 / 5 / 7, 1x3, 3x1; stride 1 and 2; explicit pad_t / pad_l with Ho / Wo that are not 'SAME'
# (the full correlation k - 1 - pad of the stride-1 input gradient; the even sub-filters of the polyphase form); N = 2
# ---------------------------------------------------------------------------------------------------------------------------------
def geometry_cases():
    cases = []
    base = [(1, 1, (7, 9)), (1, 2, (15, 16)), (3, 1, (17, 33)), (3, 2, (33, 17)), (5, 1, (8, 15)), (5, 2, (16, 9)), (7, 1, (9, 8)), (7, 2, (33, 33)),
            ((1, 3), 1, (1, 17)), ((3, 1), 2, (17, 1)), ((1, 3), 2, (16, 33)), ((3, 1), 1, (33, 16))]
    for i, (k, stride, (h, w)) in enumerate(base):
        for kernel, algo in (("dma", "mfma"), ("reg", "reg")):
            c1 = (8, 32)[(i + (kernel == "reg")) % 2]
            tag = "k%s_s%d" % (k if isinstance(k, int) else "%dx%d" % k, stride)
            cases.append(fc("geo_%s_%s_%d_32_2x%dx%d_%s" % (kernel, tag, c1, h, w, MODES[i % 3]), algo, 2, h, w, c1, 0, 32, k, stride, mode=MODES[i % 3],
                            epi=EPILOGUES[i % len(EPILOGUES)]))
    # explicit padding: (k, pad, out - in) -- the full correlation of a 3x3 / 5x5 / 7x7 gradient conv, sub-filters of 4x4, 4x3, 3x4, 2x1 taps
    # with the pads the polyphase form gives them, an output one short / one long of the input
    explicit = [(3, (2, 2), (2, 2)), (5, (4, 4), (4, 4)), (7, (3, 6), (0, 6)), ((4, 4), (2, 2), (1, 1)), ((4, 3), (1, 1), (0, 0)), ((3, 4), (1, 2), (0, 1)),
                ((2, 1), (1, 0), (1, 0)), ((2, 2), (0, 0), (-1, -1)), ((4, 4), (1, 1), (0, -1))]
    for i, (k, pad, grow) in enumerate(explicit):
        h, w = SIZES[(3 * i + 1) % len(SIZES)]
        h, w = max(h, 2), max(w, 2)
        for kernel, algo in (("dma", "mfma"), ("reg", "reg")):
            c1 = (32, 8)[(i + (kernel == "reg")) % 2]
            kh, kw = (k, k) if isinstance(k, int) else k
            cases.append(fc("geo_%s_pad_k%dx%d_p%d%d_%d_32_2x%dx%d_%s" % (kernel, kh, kw, pad[0], pad[1], c1, h, w, MODES[i % 3]), algo, 2, h, w, c1, 0, 32, k,
                            mode=MODES[i % 3], pad=pad, out=(h + grow[0], w + grow[1])))
    return cases


GEOMETRY = geometry_cases()


@pytest.mark.parametrize("o", GEOMETRY)
def test_geometry(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# output forms: cout_valid < Cout with y_cstride > cout_valid (the vector and the scalar epilogue), res_cstride > cout_valid,
# y_pix_stride = 2 with the four offsets, per-image filters; the untouched words of y keep their guard pattern
# ---------------------------------------------------------------------------------------------------------------------------------
def output_cases():
    cases = []
    for kernel, algo in (("dma", "mfma"), ("reg", "reg")):
        cases += [
            fc("out_%s16_cv8_of_16_ycs12_8_1x17x15_fx_res" % kernel, algo, 1, 17, 15, 8, 0, 16, 3, mode="fx", epi="res", cv=8, ycs=12, res_pad=4),
            fc("out_%s16_cv3_of_16_ycs5_16_2x9x17_fw_res" % kernel, algo, 2, 9, 17, 16, 0, 16, 3, mode="fw", epi="res", cv=3, ycs=5, res_pad=2),
            fc("out_%s16_cv6_of_16_ycs7_12_1x16x16_int_affine" % kernel, algo, 1, 16, 16, 12, 0, 16, 5, epi="affine", cv=6, ycs=7),
            fc("out_%s32_cv20_of_32_ycs24_32_1x15x33_fx_act2" % kernel, algo, 1, 15, 33, 32, 0, 32, 3, mode="fx", epi="act2", cv=20, ycs=24),
            fc("out_%s32_cv17_of_32_ycs17_32_2x8x9_int_res" % kernel, algo, 2, 8, 9, 32, 0, 32, 1, epi="res", cv=17, res_pad=0),
            fc("out_%s32_ycs40_32_1x9x17_fw_relu" % kernel, algo, 1, 9, 17, 32, 0, 32, 3, mode="fw", epi="relu", ycs=40),
            fc("out_%s64_cv33_of_64_ycs36_32_1x7x16_fx" % kernel, algo, 1, 7, 16, 32, 0, 64, 3, mode="fx", cv=33, ycs=36),
        ]
        for i, off in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            h, w = SIZES[(i + 2) % len(SIZES)]
            cases.append(fc("out_%s32_pix2_off%d%d_32_2x%dx%d_%s_res" % (kernel, off[0], off[1], h, w, MODES[i % 3]), algo, 2, h, w, 32, 0, 32, 3, mode=MODES[i % 3],
                            epi="res", ypix=(2, off)))
            cases.append(fc("out_%s16_pix2_off%d%d_cv5_of_16_1x%dx%d_%s" % (kernel, off[0], off[1], w, h, MODES[(i + 1) % 3]), algo, 1, w, h, 8, 0, 16, (4, 3),
                            mode=MODES[(i + 1) % 3], cv=5, ycs=6, ypix=(2, off), pad=(1, 1), out=(w, h)))
    # per-image filters: a 16-"image" 1x1 problem, as the planes plan issues it (the LDS-DMA kernel, never the register-A kernel)
    cases += [fc("wbs_16_images_32_16_16x3x16_fw", "exact", 16, 3, 16, 32, 0, 16, 1, mode="fw", wbs=True),
              fc("wbs_16_images_128_64_16x8x16_fx", "exact", 16, 8, 16, 128, 0, 64, 1, mode="fx", wbs=True),
              fc("wbs_16_images_16_16_reg_16x1x16_int", "reg", 16, 1, 16, 16, 0, 16, 1, wbs=True)]
    return cases


OUTPUT_FORMS = output_cases()


@pytest.mark.parametrize("o", OUTPUT_FORMS)
def test_output_forms(K, lib, o, monkeypatch):
    run_forward(K, lib, o, monkeypatch)


# every epilogue on the staged store (BN >= 32, every channel stored), the accumulator-layout store (BN = 16; SHDR_CONV_LEGACY_EPILOGUE),
# the register-staged kernel, the register-A kernel and the direct kernel
def epilogue_cases():
    cases = []
    for i, epi in enumerate(EPILOGUES):
        h, w = SIZES[(i + 4) % len(SIZES)]
        m = MODES[i % 3]
        cases += [fc("epilogue_dma64_%s_32_64_1x%dx%d_%s" % (epi, h, w, m), "mfma", 1, h, w, 32, 0, 64, 3, mode=m, epi=epi),
                  fc("epilogue_dma32_%s_8_32_2x%dx%d_%s" % (epi, h, w, m), "mfma", 2, h, w, 8, 0, 32, 3, mode=m, epi=epi),
                  fc("epilogue_dma16_%s_16_16_1x%dx%d_%s" % (epi, w, h, m), "mfma", 1, w, h, 16, 0, 16, 3, mode=m, epi=epi),
                  fc("legacy_dma64_%s_32_64_1x%dx%d_%s" % (epi, h, w, m), "mfma", 1, h, w, 32, 0, 64, 3, mode=m, epi=epi, env={"SHDR_CONV_LEGACY_EPILOGUE": "1"}),
                  fc("epilogue_reg_%s_16_16_32_1x%dx%d_%s" % (epi, h, w, m), "mfma", 1, h, w, 16, 16, 32, 3, mode=m, epi=epi, x2s=0.5),
                  fc("epilogue_rega_%s_16_16_2x%dx%d_%s" % (epi, h, w, m), "exact", 2, h, w, 16, 0, 16, 5, mode=m, epi=epi),
                  fc("epilogue_direct_%s_6_5_1x%dx%d_%s" % (epi, w, h, m), "exact", 1, w, h, 6, 0, 5, 3, mode=m, epi=epi, res_pad=1)]
    return cases


EPILOGUE_CASES = epilogue_cases()


@pytest.mark.parametrize("o", EPILOGUE_CASES)
def test_epilogues(K, lib, o, monkeypatch):
    kind = o["name"].split("_")[1]
    want = {"dma64": "conv_mfma_dma_kernel<128, 64", "dma32": "conv_mfma_dma_kernel<128, 32", "dma16": "conv_mfma_dma_kernel<128, 16",
            "reg": "conv_mfma_kernel<128, 32", "rega": "conv_rega_kernel<4, 1, 16, 5>", "direct": "conv_direct_kernel<8>"}[kind]
    assert want in instance(o), instance(o)
    run_forward(K, lib, o, monkeypatch)


def first(cases, prefix):
    return next(p for p in cases if p.id.startswith(prefix))


@pytest.mark.parametrize("o", [first(EPILOGUE_CASES, "epilogue_%s_relu" % k) for k in ("dma64", "dma16", "reg", "rega", "direct")])
def test_range_slot_presets(K, lib, o, monkeypatch):
    """an empty slot receives max |y|; a larger preset survives; a smaller one is raised -- from the staged and the accumulator-layout
    epilogue (one atomic per block), the register-A kernel (one per wave and tile) and the pass over y behind the direct kernel"""
    r = reference(o)
    for preset in (0.0, 1.0e6, float(np.float32(r["ymax"]) / 2)):
        run_forward(K, lib, o, monkeypatch, r=r, preset=preset)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_rega_kernel<4, NT, CT, KK>: NT 1 / 2 (Cout 16 / 32), CT 4, 16 (C1 8 / 12 / 16), 32 (16 + 16, with and without x2_scale), KK 3 / 5 / 7,
# KK 0 through a non-square filter and through SHDR_REGA_NO_DPP; W from {1, 15, 16, 17, 18, 33} (the DPP halo lanes fi < KK - 1 and the
# column iw0 + 16); <4, 4, 4, 3>; the persistent loop; the refusal at the 100 KB bound
# ---------------------------------------------------------------------------------------------------------------------------------
REGA_W = (1, 15, 16, 17, 18, 33)


def rega_cases():
    cases, i = [], 0
    for k in (3, 5, 7):
        for c1, c2 in ((4, 0), (8, 0), (12, 0), (16, 0), (16, 16)):
            for cout in (16, 32):
                if k * k * (c1 + c2) * cout * 4 > 100 * 1024:
                    continue                                              # refused: tested below
                i += 1
                w, h = REGA_W[i % 6], (17, 4, 33, 16, 5)[i % 5]
                x2s = (1.0, S4)[i % 2] if c2 else 1.0
                name = "rega_k%d_%d_%d_%d_%dx%dx%d_%s_%s" % (k, c1, c2, cout, 1 + i % 2, h, w, MODES[i % 3], EPILOGUES[i % len(EPILOGUES)])
                cases.append(fc(name, "exact", 1 + i % 2, h, w, c1, c2, cout, k, mode=MODES[i % 3], epi=EPILOGUES[i % len(EPILOGUES)], x2s=x2s))
    for j, (c1, c2, cout) in enumerate(((4, 0, 16), (12, 0, 32), (16, 16, 16), (16, 0, 32), (16, 16, 32), (4, 0, 32))):
        w = REGA_W[(2 * j + 1) % 6]
        cases.append(fc("rega_k1x3_%d_%d_%d_2x9x%d_%s" % (c1, c2, cout, w, MODES[j % 3]), "exact", 2, 9, w, c1, c2, cout, (1, 3), mode=MODES[j % 3],
                        x2s=0.5 if c2 else 1.0))
        cases.append(fc("rega_nodpp_k3_%d_%d_%d_1x17x%d_%s" % (c1, c2, cout, w, MODES[(j + 1) % 3]), "exact", 1, 17, w, c1, c2, cout, 3, mode=MODES[(j + 1) % 3],
                        epi="relu", env={"SHDR_REGA_NO_DPP": "1"}))
    cases += [fc("rega_k5x3_8_0_16_1x16x18_fx", "exact", 1, 16, 18, 8, 0, 16, (5, 3), mode="fx"),
              fc("rega_image64_4_64_2x17x33_fx_relu", "exact", 2, 17, 33, 4, 0, 64, 3, mode="fx", epi="relu"),
              fc("rega_image64_4_64_1x16x18_fw_res", "exact", 1, 16, 18, 4, 0, 64, 3, mode="fw", epi="res"),
              fc("rega_image64_4_64_1x1x1_int", "exact", 1, 1, 1, 4, 0, 64, 3),
              # explicit padding and a strided, channel-padded output on the register-A kernel (the gradient convs of the narrow layers)
              fc("rega_pad_k5_p44_16_0_16_1x9x15_fw", "exact", 1, 9, 15, 16, 0, 16, 5, mode="fw", pad=(4, 4), out=(13, 19)),
              fc("rega_pix2_off11_cv3_of_16_8_1x8x17_fx_res", "exact", 1, 8, 17, 8, 0, 16, 3, mode="fx", epi="res", cv=3, ycs=4, res_pad=1, ypix=(2, (1, 1)))]
    return cases


REGA = rega_cases()
REGA_REFUSED = [fc("rega_refused_k7_16_16_32_1x17x15_fx_relu", "exact", 1, 17, 15, 16, 16, 32, 7, mode="fx", epi="relu"),
                fc("rega_refused_no_rega_16_0_32_2x15x17_fw", "exact", 2, 15, 17, 16, 0, 32, 3, mode="fw", env={"SHDR_NO_REGA": "1"}),
                fc("rega_refused_k9_16_0_32_1x9x16_int", "exact", 1, 9, 16, 16, 0, 32, 9, keep=0.5)]


@pytest.mark.parametrize("o", REGA)
def test_register_a_kernel(K, lib, o, monkeypatch):
    assert "conv_rega_kernel" in instance(o), instance(o)
    run_forward(K, lib, o, monkeypatch)


@pytest.mark.parametrize("o", REGA_REFUSED)
def test_register_a_kernel_declines_and_the_dma_kernel_answers(K, lib, o, monkeypatch):
    """a filter over the 100 KB LDS bound (7x7 16 + 16 -> 32: 196 KB; 9x9 16 -> 32: 162 KB) and SHDR_NO_REGA"""
    assert "conv_mfma_dma_kernel<128, 32, 4, 1" in instance(o), instance(o)
    run_forward(K, lib, o, monkeypatch)


# the persistent loop: SHDR_REGA_PER_CU=1 gives 256 blocks, 1 x 272 x 256 has 17 x 16 = 272 tiles of 16 x 16: sixteen blocks take a second tile
REGA_PERSISTENT = [fc("rega_persistent_k3_4_0_16_1x272x256_int_relu", "exact", 1, 272, 256, 4, 0, 16, 3, epi="relu", env={"SHDR_REGA_PER_CU": "1"}),
                   fc("rega_persistent_k1x3_4_0_16_1x272x256_fx", "exact", 1, 272, 256, 4, 0, 16, (1, 3), mode="fx", env={"SHDR_REGA_PER_CU": "1"})]


@pytest.mark.parametrize("o", REGA_PERSISTENT)
def test_register_a_persistent_loop(K, lib, o, monkeypatch):
    assert -(-272 // 16) * (256 // 16) == 272 and "conv_rega_kernel<4, 1, 4" in instance(o)
    run_forward(K, lib, o, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# conv_direct_kernel<3 | 8 | 16>: Cin 3 / 6 / 9, Cout 3 / 5 / 8 / 16, operand pointers 4 bytes off a 16-byte boundary, stride 2, two sources
# with x2_scale, a strided output; the range slot through shdr_absmax_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def direct_cases():
    cases, i = [], 0
    for c1 in (3, 6, 9):
        for cout in (3, 5, 8, 16):
            i += 1
            h, w = SIZES[i % len(SIZES)]
            k = (3, 1, 5, 7, (1, 3), (3, 1))[i % 6]
            cases.append(fc("direct_%d_%d_k%s_s%d_%dx%dx%d_%s_%s" % (c1, cout, k if isinstance(k, int) else "%dx%d" % k, 1 + i % 2, 1 + i % 2, h, w, MODES[i % 3],
                                                                     EPILOGUES[i % len(EPILOGUES)]),
                            "exact", 1 + i % 2, h, w, c1, 0, cout, k, 1 + i % 2, mode=MODES[i % 3], epi=EPILOGUES[i % len(EPILOGUES)], res_pad=i % 3))
    cases += [fc("direct_two_3_6_scaled_5_2x9x17_fx_res", "exact", 2, 9, 17, 3, 6, 5, 3, mode="fx", epi="res", x2s=S4, res_pad=0),
              fc("direct_two_6_3_half_16_s2_1x17x16_fw", "exact", 1, 17, 16, 6, 3, 16, 5, 2, mode="fw", x2s=0.5),
              fc("direct_unaligned_8_16_1x15x9_fx_res", "exact", 1, 15, 9, 8, 0, 16, 3, mode="fx", epi="res", lead=1),
              fc("direct_unaligned_two_4_4_3_2x8x7_fw_affine", "exact", 2, 8, 7, 4, 4, 3, 3, mode="fw", epi="affine", x2s=0.5, lead=1),
              fc("direct_forced_16_32_1x9x8_int", "direct", 1, 9, 8, 16, 0, 32, 3),
              fc("direct_pad_k4x3_6_5_1x8x9_int", "exact", 1, 8, 9, 6, 0, 5, (4, 3), pad=(2, 1), out=(9, 9)),
              fc("direct_pix2_off10_ycs7_3_5_1x7x8_fx_res", "exact", 1, 7, 8, 3, 0, 5, 3, mode="fx", epi="res", ycs=7, ypix=(2, (1, 0)), res_pad=2, slot=False)]
    return cases


DIRECT = direct_cases()


@pytest.mark.parametrize("o", DIRECT)
def test_direct_kernel(K, lib, o, monkeypatch):
    cout = o["cout"]
    assert instance(o) == "conv_direct_kernel<%d>" % (3 if cout <= 3 else (16 if cout % 16 == 0 else 8)), instance(o)
    run_forward(K, lib, o, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------
# PREC 1 / 2: fp16 / bf16 MFMA operands, rounded to nearest-even when packed (the comment above conv_mfma_dma_kernel).  int mode is exact; a
# fine mode equals the model that rounds both operands and convolves exactly -- and differs from the unrounded one (asserted).  The
# AUTO_* rule hands single-source 4 / <= 16-channel layers with 16 (64) couts back to the exact register-A kernel: unrounded there.
# ---------------------------------------------------------------------------------------------------------------------------------
def prec_cases():
    cases, i = [], 0
    for algo in ("f16", "bf16", "auto_f16", "auto_bf16"):
        for c1, c2, cout, k in ((32, 0, 128, 3), (64, 0, 64, 1), (12, 0, 32, 3), (16, 16, 16, 3), (32, 32, 32, (1, 3)), (36, 0, 16, 5)):
            for mode in MODES:
                i += 1
                h, w = SIZES[i % len(SIZES)]
                cases.append(fc("prec_%s_%d_%d_%d_k%s_%dx%dx%d_%s" % (algo, c1, c2, cout, k if isinstance(k, int) else "%dx%d" % k, 1 + i % 2, h, w, mode), algo,
                                1 + i % 2, h, w, c1, c2, cout, k, 1 + (i % 5 == 0), mode=mode, epi=EPILOGUES[i % len(EPILOGUES)]))
    for algo in ("auto_f16", "auto_bf16"):
        cases += [fc("prec_%s_rega_k7_4_16_1x15x17_fx" % algo, algo, 1, 15, 17, 4, 0, 16, 7, mode="fx"),
                  fc("prec_%s_rega_k3_16_16_2x17x16_fw_relu" % algo, algo, 2, 17, 16, 16, 0, 16, 3, mode="fw", epi="relu"),
                  fc("prec_%s_rega_image64_1x16x33_fx" % algo, algo, 1, 16, 33, 4, 0, 64, 3, mode="fx"),
                  # ... but not the 32-cout and 16 + 16 layers, which stay on the reduced-precision LDS-DMA kernel
                  fc("prec_%s_dma_k3_16_32_1x17x15_fx" % algo, algo, 1, 17, 15, 16, 0, 32, 3, mode="fx"),
                  fc("prec_%s_dma_k5_16_16_16_1x9x17_fw" % algo, algo, 1, 9, 17, 16, 16, 16, 5, mode="fw"),
                  # x2_scale != 1: the AUTO modes fall back to exact operands on the register-staged kernel
                  fc("prec_%s_exact_x2s_32_32_32_1x15x16_fx" % algo, algo, 1, 15, 16, 32, 32, 32, 3, mode="fx", x2s=0.5)]
    return cases


PREC = prec_cases()


@pytest.mark.parametrize("o", PREC)
def test_reduced_precision_operands(K, lib, o, monkeypatch):
    prec, name = precision(o), instance(o)
    tag = o["name"].split("_")
    if "rega" in tag:
        assert prec == 0 and "conv_rega_kernel" in name, name
    elif "exact" in tag:
        assert prec == 0 and "conv_mfma_kernel" in name, name
    else:
        assert prec == (1 if "f16" in tag[1:3] and "bf16" not in tag[1:3] else 2) and name.endswith(", %d>" % prec), (name, prec)
    r = reference(o)
    if o["mode"] != "int":                                               # the other precision's model differs somewhere: the check can tell them apart
        assert not np.array_equal(r["y"], reference(o, wrong="f16")["y"])
    run_forward(K, lib, o, monkeypatch, r=r)


# ---------------------------------------------------------------------------------------------------------------------------------
# winograd_fused_kernel<R, UP>: shdr_conv2d_winograd_fused2_f32 / _fused_f32 / _fused_up2_f32
# ---------------------------------------------------------------------------------------------------------------------------------
def wc(name, n, h, w, c1, c2, cout, mode="int", epi="plain", **o):
    o.update(name=name, n=n, h=h, w=w, c1=c1, c2=c2, cout=cout, mode=mode, epi=epi, kh=3, kw=3, stride=1, x2s=1.0, algo="exact")
    o.setdefault("env", {})
    return pytest.param(o, id=name)


WF_SIZES = [(1, 1), (2, 2), (7, 9), (8, 16), (9, 15), (15, 17), (16, 18), (17, 33), (18, 8), (33, 7), (1, 18), (2, 33)]     # from {1,2,7,8,9,15,16,17,18,33}^2
WF_EPI = [e for e in EPILOGUES if e != "res"]                               # (the fused kernel takes no residual)


def wino_cases():
    cases, i = [], 0
    for tag, env in (("wf", {}), ("wf16", {"SHDR_WINOGRAD_TILE": "16"})):
        # one chunk (8), several (24, 32), more than the four-buffer pipeline holds (72); one and two cout slices; two sources 8 + 8, 16 + 16
        for c1, c2 in ((8, 0), (24, 0), (32, 0), (72, 0), (8, 8), (16, 16)):
            for cout in (64, 128):
                i += 1
                (h, w), n = WF_SIZES[i % len(WF_SIZES)], 1 + i % 2
                keep = 0.5 if c1 == 72 else 1.0
                cases.append(wc("%s_%d_%d_%d_%dx%dx%d_%s_%s" % (tag, c1, c2, cout, n, h, w, MODES[i % 3], WF_EPI[i % len(WF_EPI)]), n, h, w, c1, c2, cout,
                                mode=MODES[i % 3], epi=WF_EPI[i % len(WF_EPI)], env=env, keep=keep))
        # pooled outputs: y_pool with y, y_pool alone
        for j, (pool, (h, w), c1, c2, cout) in enumerate((("with_y", (2, 2), 8, 0, 64), ("with_y", (16, 18), 24, 0, 128), ("only", (8, 34), 16, 16, 64),
                                                         ("only", (18, 16), 32, 0, 64))):
            cases.append(wc("%s_pool_%s_%d_%d_%d_2x%dx%d_%s_relu" % (tag, pool, c1, c2, cout, h, w, MODES[j % 3]), 2, h, w, c1, c2, cout, mode=MODES[j % 3], epi="relu",
                            env=env, pool=pool))
    # the remaining sizes on R = 1, one-source entry point
    for j, (h, w) in enumerate(WF_SIZES):
        cases.append(wc("wf_entry1_32_0_64_1x%dx%d_%s" % (h, w, MODES[j % 3]), 1, h, w, 32, 0, 64, mode=MODES[j % 3], epi=WF_EPI[j % len(WF_EPI)], entry=1))
    # UP: the low-res sizes 1x1, 1x2, 4x8, 5x9; int and fw (a fine x does not survive the resize); 8, 24, 72 channels: one chunk, several, more
    # than the five-buffer ring holds
    for j, ((h, w), c1, cout, mode) in enumerate((((1, 1), 8, 64, "fw"), ((1, 2), 24, 64, "int"), ((4, 8), 72, 128, "int"), ((5, 9), 32, 64, "int"),
                                                  ((5, 9), 72, 64, "int"), ((4, 8), 8, 128, "fw"), ((1, 2), 72, 128, "int"), ((5, 9), 24, 128, "fw"))):
        cases.append(wc("wfup_%d_%d_%dx%dx%d_%s_%s" % (c1, cout, 1 + j % 2, h, w, mode, WF_EPI[j % len(WF_EPI)]), 1 + j % 2, h, w, c1, 0, cout,
                        mode=mode, epi=WF_EPI[j % len(WF_EPI)], up=True, keep=0.25 if mode == "fw" else 1.0))
    return cases


WINO = wino_cases()


def wino_reference(o, wrong=None, probe=False):
    """conv_ref.conv2d of the (up-sampled) input -- and, asserted, conv_ref.winograd_conv of it, with the transform-domain bounds"""
    x, x2, wt = operands(o)
    xin = x
    if o.get("up"):
        x = x * 16.0                                                     # multiples of 16: both lerps of the resize are exact
        xin = C.resize2x(x.astype(np.float32)).astype(np.float64)
        assert np.array_equal(xin, C.resize2x(x)), "the fp32 resize must be exact on these operands"
    oo = dict(o, h=xin.shape[1], w=xin.shape[2])
    z, total, lsb = model(oo, xin, x2, wt, wrong, probe)
    if probe:
        return dict(y=z)
    assert float(total.max()) / lsb < LIMIT
    if wrong is None:
        zw, gemm, out = C.winograd_conv(xin, x2, wt)
        assert gemm < LIMIT and out < LIMIT, "%s: transform-domain sums %.3g / %.3g of 2^24" % (o["name"], gemm / LIMIT, out / LIMIT)
        assert np.array_equal(zw, z), "Winograd by its definition IS the convolution on these operands"
    bias, act1, scale, shift, res, act2 = epilogue_operands(o["name"], o["epi"], o["cout"], z.shape[:3])
    y = C.epilogue(z + (0.0 if bias is None else bias), act1, scale, shift, None, act2)
    r = dict(x=x, x2=x2, w=wt, bias=bias, act1=act1, scale=scale, shift=shift, act2=act2, y=y, H=xin.shape[1], W=xin.shape[2])
    if o.get("pool"):
        r["yp"] = C.maxpool2(y)
    return r


def packed_filter(K, lib, wd, cin, cout):
    u = torch.empty(16 * cin * cout, device="cuda")
    assert lib.shdr_winograd_filter_packed_f32(P(wd), P(u), cin, cout, K._stream()) == 0, lib.shdr_last_error()
    return u


@pytest.mark.parametrize("o", WINO)
def test_fused_winograd(K, lib, o, monkeypatch):
    for name, value in o["env"].items():
        monkeypatch.setenv(name, value)
    r = wino_reference(o)
    n, c1, c2, cout, H, W = o["n"], o["c1"], o["c2"], o["cout"], r["H"], r["W"]
    rr = 2 if o["env"] else 1
    what = "%s [winograd_fused_kernel<%d%s>]" % (o["name"], rr, ", true" if o.get("up") else "")
    xd, wd = dev(r["x"]), dev(r["w"])
    x2d = None if r["x2"] is None else dev(r["x2"])
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift")}
    u = packed_filter(K, lib, wd, c1 + c2, cout)
    y = None if o.get("pool") == "only" else Out((n, H, W, cout))
    yp = Out((n, H // 2, W // 2, cout)) if o.get("pool") else None
    st = K._stream()
    if o.get("up"):
        rc = lib.shdr_conv2d_winograd_fused_up2_f32(P(xd), P(u), P(opt["bias"]), P(opt["scale"]), P(opt["shift"]), y.ptr, n, H, W, c1, cout, r["act1"], r["act2"], st)
    elif o.get("entry") == 1:
        rc = lib.shdr_conv2d_winograd_fused_f32(P(xd), P(u), P(opt["bias"]), P(opt["scale"]), P(opt["shift"]), y.ptr, n, H, W, c1, cout, r["act1"], r["act2"], st)
    else:
        rc = lib.shdr_conv2d_winograd_fused2_f32(P(xd), P(x2d), P(u), P(opt["bias"]), P(opt["scale"]), P(opt["shift"]), y.ptr if y else None,
                                                 yp.ptr if yp else None, n, H, W, c1, c2, cout, r["act1"], r["act2"], st)
    assert rc == 0, (what, rc, lib.shdr_last_error())
    if y is not None:
        same_in_tiles(y.words(what + " y").view(np.float32), r["y"], what + " y", (8 * rr, 16))
    if yp is not None:
        same_in_tiles(yp.words(what + " pooled output").view(np.float32), r["yp"], what + " pooled output", (4 * rr, 8))


# ---------------------------------------------------------------------------------------------------------------------------------
# the transform kernels of the planes plan, each against its definition: U = G g G^T (plain and in the packed operand order), V = B^T d B,
# Y = A^T M A (+ epilogue)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,mode", [(8, 64, "fw"), (24, 128, "int"), (72, 64, "fw"), (12, 16, "fw"), (128, 272, "int")])
def test_winograd_filter_transforms(K, lib, cin, cout, mode):
    rng = np.random.default_rng(seed_of("wino_filter_%d_%d" % (cin, cout)))
    w = fine_w(rng, (3, 3, cin, cout))[0] if mode == "fw" else int_w(rng, (3, 3, cin, cout))
    u = C.winograd_filter(w)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    wd = dev(w)
    out = Out((16, cin, cout))
    assert lib.shdr_winograd_filter_f32(P(wd), out.ptr, cin, cout, K._stream()) == 0, lib.shdr_last_error()
    same(out.words("winograd_filter").view(np.float32), u, "winograd_filter %d -> %d" % (cin, cout))
    if cin % 8 == 0 and cout % 64 == 0:
        packed = Out((16 * cin * cout,))
        assert lib.shdr_winograd_filter_packed_f32(P(wd), packed.ptr, cin, cout, K._stream()) == 0, lib.shdr_last_error()
        want = np.empty(16 * cin * cout)
        want[C.winograd_packed_index(cin, cout).reshape(-1)] = u.reshape(-1)
        same(packed.words("winograd_filter_packed").view(np.float32), want, "winograd_filter_packed %d -> %d" % (cin, cout))


@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 4), (2, 3, 5, 8), (1, 17, 33, 12), (2, 16, 16, 4), (1, 2, 7, 128)])
def test_winograd_input_and_output_transforms(K, lib, n, h, w, c):
    rng = np.random.default_rng(seed_of("wino_io_%d_%d_%d_%d" % (n, h, w, c)))
    tiles, rows = C.winograd_rows(n, h, w)
    assert rows == int(lib.shdr_winograd_tiles(n, h, w)) and rows % 128 == 0 and rows >= tiles
    # V = B^T d B: the rows of the tiles; the padding rows of every plane are not written
    x = fine_x(rng, (n, h, w, c))[0]
    out = Out((16, rows, c))
    xd = dev(x)
    assert lib.shdr_winograd_input_f32(P(xd), out.ptr, n, h, w, c, K._stream()) == 0, lib.shdr_last_error()
    words = out.words("winograd_input")
    same(np.ascontiguousarray(words[:, :tiles]).view(np.float32), C.winograd_input(x), "winograd_input %dx%dx%dx%d" % (n, h, w, c))
    assert (words[:, tiles:] == SENT32).all(), "winograd_input wrote the padding rows of a plane"
    # Y = A^T M A + the epilogue, from planes whose padding rows hold NaN
    m = rng.integers(-4, 5, size=(16, tiles, c)).astype(np.float64)
    mfull = np.full((16, rows, c), np.nan)
    mfull[:, :tiles] = m
    md = torch.from_numpy(mfull.astype(np.float32)).cuda()
    for epi in ("plain", "affine", "act2"):
        bias, act1, scale, shift, _, act2 = epilogue_operands("wino_out_%s" % epi, epi, c, (n, h, w))
        yo = Out((n, h, w, c))
        opt = [None if v is None else dev(v) for v in (bias, scale, shift)]
        assert lib.shdr_winograd_output_f32(P(md), yo.ptr, P(opt[0]), P(opt[1]), P(opt[2]), n, h, w, c, act1, act2, K._stream()) == 0, lib.shdr_last_error()
        want = C.epilogue(C.winograd_output(m, n, h, w) + bias, act1, scale, shift, None, act2)
        same(yo.words("winograd_output").view(np.float32), want, "winograd_output %dx%dx%dx%d %s" % (n, h, w, c, epi))


# ---------------------------------------------------------------------------------------------------------------------------------
# the planes plan through shdr_conv2d_fwd_prepared_ranged_f32.  plan_of gives WINOGRAD_PLANES to the wide layers the fused kernel cannot
# take -- Cout off the 64 grid, Cin Cout >= 32768 -- so 128 -> 272 and 128 -> 304 reach it; 128 -> 128 and 128 -> 256 plan the fused kernel (asserted) and
# are run BOTH through the planned call and as the three launches of the planes plan by hand (input transform, the 16-"image" 1x1 GEMM
# with w_batch_stride on conv_mfma_dma_kernel, output transform).  1x1, 3x5 (far below one 128-row GEMM tile) and 17x33 (153 tiles).
# ---------------------------------------------------------------------------------------------------------------------------------
PLANES = [wc("planes_128_%d_1x%dx%d_%s_%s" % (cout, h, w, mode, epi), 1, h, w, 128, 0, cout, mode=mode, epi=epi, keep=0.5)
          for cout, (h, w), mode, epi in ((128, (1, 1), "fw", "plain"), (128, (3, 5), "fx", "relu"), (128, (17, 33), "int", "affine"),
                                          (256, (1, 1), "int", "lrelu"), (256, (3, 5), "fw", "act2"), (256, (17, 33), "fx", "nobias"),
                                          (272, (1, 1), "fx", "affine"), (272, (3, 5), "fw", "plain"), (272, (17, 33), "int", "act2"),
                                          (304, (3, 5), "int", "nobias"), (304, (17, 33), "fw", "relu"))]


@pytest.mark.parametrize("o", PLANES)
def test_planes_plan(K, lib, o, monkeypatch):
    r = wino_reference(o)
    n, h, w, cin, cout = o["n"], o["h"], o["w"], o["c1"], o["cout"]
    name, st = o["name"], K._stream()
    d = K._conv_desc((n, h, w, cin), (3, 3, cin, cout), 1, 0, 1.0, None)
    d.act1, d.act2, d.algo, d.y_cstride = r["act1"], r["act2"], ALGO["exact"], cout
    plan = PLAN[int(lib.shdr_conv2d_plan_f32(ctypes.byref(d), 0))]
    assert plan == plan_expected(o) == ("fused" if cout % 64 == 0 else "planes"), (name, plan)
    xd, wd = dev(r["x"]), dev(r["w"])
    opt = {f: (None if r[f] is None else dev(r[f])) for f in ("bias", "scale", "shift")}
    # the planned call: prepared filter, workspace of exactly the bytes asked for between guards, y_range through the pass over y
    prepared = torch.empty(int(lib.shdr_conv2d_prepared_filter_elems_f32(ctypes.byref(d), 0)), device="cuda")
    assert lib.shdr_conv2d_prepare_filter_f32(ctypes.byref(d), 0, P(wd), P(prepared), st) == 0, lib.shdr_last_error()
    nbytes = int(lib.shdr_conv2d_workspace_bytes_f32(ctypes.byref(d), 0))
    assert nbytes % 4 == 0 and (nbytes > 0) == (plan == "planes")
    ws = Out((max(nbytes // 4, 4),))
    y, slot = Out((n, h, w, cout)), Slot(0.0)
    rc = lib.shdr_conv2d_fwd_prepared_ranged_f32(ctypes.byref(d), P(xd), None, P(prepared), P(opt["bias"]), P(opt["scale"]), P(opt["shift"]), None, y.ptr, None,
                                                 ws.ptr, None, None, P(slot.view), st)
    assert rc == 0, (name, rc, lib.shdr_last_error())
    ws.words(name + " workspace")
    same_in_tiles(y.words(name + " y").view(np.float32), r["y"], "%s y [plan %s]" % (name, plan), (2, 2) if plan == "planes" else (8, 16))
    slot.check(float(np.abs(r["y"]).max()), name)
    # the three launches by hand
    tiles, rows = C.winograd_rows(n, h, w)
    u, v, m = Out((16, cin, cout)), Out((16, rows, cin)), Out((16, rows, cout))
    # (the padding rows of V keep the guards' NaN pattern: a GEMM row depends on its own row of V only)
    assert lib.shdr_winograd_filter_f32(P(wd), u.ptr, cin, cout, st) == 0 and lib.shdr_winograd_input_f32(P(xd), v.ptr, n, h, w, cin, st) == 0
    g = K._conv_desc((16, rows // 16, 16, cin), (1, 1, cin, cout), 1, 0, 1.0, None)
    g.algo, g.w_batch_stride = ALGO["auto"], cin * cout
    assert lib.shdr_conv2d_fwd_f32(ctypes.byref(g), v.ptr, None, u.ptr, None, None, None, None, m.ptr, st) == 0, lib.shdr_last_error()
    mw = np.ascontiguousarray(m.words(name + " M")[:, :tiles]).view(np.float32)
    want_m = np.einsum("xtc,xco->xto", C.winograd_input(r["x"]), C.winograd_filter(r["w"]))
    same(mw, want_m, name + " M = V @ U [conv_mfma_dma_kernel on 16 images with per-image filters]")
    y2 = Out((n, h, w, cout))
    assert lib.shdr_winograd_output_f32(m.ptr, y2.ptr, P(opt["bias"]), P(opt["scale"]), P(opt["shift"]), n, h, w, cout, r["act1"], r["act2"], st) == 0
    same_in_tiles(y2.words(name + " y by hand").view(np.float32), r["y"], name + " y by hand", (2, 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# shdr_conv2d_dgrad_ranged_f32 with algo = SHDR_ALGO_AUTO_EXACT
# ---------------------------------------------------------------------------------------------------------------------------------
def dc(name, kind, n, h, w, c1, c2, cout, k, stride, which=0, mode="int", **o):
    kh, kw = (k, k) if isinstance(k, int) else k
    o.update(name=name, kind=kind, n=n, h=h, w=w, c1=c1, c2=c2, cout=cout, kh=kh, kw=kw, stride=stride, which=which, mode=mode)
    o.setdefault("x2s", 1.0)
    o.setdefault("env", {})
    return pytest.param(o, id=name)


def dgrad_cases():
    cases = [
        # stride 1, the fused Winograd kernel on dz (Cx % 64 == 0, dz channels % 8 == 0 and >= 32): no dx_range
        dc("dgrad_wino_cx64_from_32_1x17x15_fx", "wino", 1, 17, 15, 64, 0, 32, 3, 1, mode="fx"),
        dc("dgrad_wino_two_64_64_which1_scaled_from_40_2x9x16_fw", "wino", 2, 9, 16, 64, 64, 40, 3, 1, which=1, mode="fw", x2s=S4),
        # stride 1, the MFMA kernels: Cx off the 16 grid (CC padded; only c_count channels of dx written), cout_valid % 4 != 0 (the pad_dz copy)
        dc("dgrad_mfma_cx3_from_16_1x17x15_fx", "mfma", 1, 17, 15, 3, 0, 16, 3, 1, mode="fx"),
        dc("dgrad_mfma_cx20_from_32_k5_2x9x16_fw", "mfma", 2, 9, 16, 20, 0, 32, 5, 1, mode="fw"),
        dc("dgrad_mfma_two_4_6_which1_scaled_from_64_k3_1x16x17_int", "mfma", 1, 16, 17, 4, 6, 64, 3, 1, which=1, x2s=S4),
        dc("dgrad_mfma_cx16_from_3_of_16_k7_1x15x15_fx", "mfma", 1, 15, 15, 16, 0, 16, 7, 1, mode="fx", cv=3),
        dc("dgrad_mfma_cx64_from_5_of_16_k3_1x8x33_fw", "mfma", 1, 8, 33, 64, 0, 16, 3, 1, mode="fw", cv=5),
        dc("dgrad_mfma_cx64_from_30_of_32_k3_1x9x9_int", "mfma", 1, 9, 9, 64, 0, 32, 3, 1, cv=30),
        dc("dgrad_mfma_cx64_from_64_k1_1x7x17_fx", "mfma", 1, 7, 17, 64, 0, 64, 1, 1, mode="fx"),
        dc("dgrad_mfma_cx32_from_32_k1x3_1x7x17_fw", "mfma", 1, 7, 17, 32, 0, 32, (1, 3), 1, mode="fw"),
    ]
    # 1x1 / 2: the coarse grid, the rest of dx exactly zero
    for i, (h, w) in enumerate(((1, 1), (2, 2), (15, 16), (17, 15), (16, 17))):
        cases.append(dc("dgrad_1x1s2_%d_from_%d_%dx%dx%d_%s" % ((64, 24)[i % 2], (32, 64)[i % 2], 1 + i % 2, h, w, MODES[i % 3]), "1x1s2", 1 + i % 2, h, w, (64, 24)[i % 2],
                        0, (32, 64)[i % 2], 1, 2, mode=MODES[i % 3]))
    # polyphase: 3x3 / 2 and 7x7 / 2 at H, W from {1, 2, 15, 16, 17}: both 'SAME' paddings (odd sizes pad k // 2 before, even ones one less),
    # all four phases, phases without pixels (H = 1 or W = 1)
    for k in (3, 7):
        for i, (h, w) in enumerate(((1, 1), (1, 2), (2, 1), (2, 2), (15, 16), (16, 15), (17, 17), (16, 16), (17, 2), (1, 17))):
            cx, cz = ((4, 16), (16, 32), (3, 16), (32, 64))[(i + k) % 4]
            cases.append(dc("dgrad_poly_k%d_cx%d_from_%d_%dx%dx%d_%s" % (k, cx, cz, 1 + i % 2, h, w, MODES[(i + k) % 3]), "poly", 1 + i % 2, h, w, cx, 0, cz, k, 2,
                            mode=MODES[(i + k) % 3], keep=0.5 if k == 7 else 1.0))
    cases += [dc("dgrad_poly_k3_two_8_4_which1_scaled_from_16_1x15x17_fx", "poly", 1, 15, 17, 8, 4, 16, 3, 2, which=1, mode="fx", x2s=S4),
              dc("dgrad_poly_k7_two_4_16_which1_half_from_6_of_16_2x16x17_fw", "poly", 2, 16, 17, 4, 16, 16, 7, 2, which=1, mode="fw", x2s=0.5, cv=6, keep=0.5),
              dc("dgrad_poly_k5x3_cx8_from_16_1x16x15_int", "poly", 1, 16, 15, 8, 0, 16, (5, 3), 2)]
    return cases


DGRAD = dgrad_cases()


def dgrad_reference(o, wrong=None, probe=False):
    """conv_ref.dgrad in float64 on exact operands; the precondition on the terms of the gradient convolution"""
    n, h, w, c1, c2, cout, kh, kw, stride, which, x2s = (o[f] for f in ("n", "h", "w", "c1", "c2", "cout", "kh", "kw", "stride", "which", "x2s"))
    cv = o.get("cv") or cout
    rng = np.random.default_rng(seed_of(o["name"]))
    ho, wo = -(-h // stride), -(-w // stride)
    keep = o.get("keep", 1.0)
    dz = fine_x(rng, (n, ho, wo, cv), keep)[0] if o["mode"] == "fx" else int_x(rng, (n, ho, wo, cv), keep)[0]
    shape = (kh, kw, c1 + c2, cout)
    wt = fine_w(rng, shape, keep, cv if cv != cout else None)[0] if o["mode"] == "fw" else int_w(rng, shape, keep, cv if cv != cout else None)
    if probe:
        dz, wt = np.ones_like(dz), np.ones_like(wt)
    cb, cc, s = (c1, c2, x2s) if which else (0, c1, 1.0)
    if wrong == "tap":
        wt = wt.copy()
        wt[C.same_pad(h, kh, stride)[1], C.same_pad(w, kw, stride)[1]] = 0.0      # the tap through which x[0, 0] reaches z[0, 0]
    if wrong == "swap":                                                   # the other source's filter rows (or rows one channel off)
        cb = (0 if which else c1) if c1 == c2 else cb + (-1 if which else 1)
    dx = C.dgrad(dz, wt[..., :cv], (n, h, w, cc), cb, cc, s, stride)
    total = C.dgrad(np.abs(dz), np.abs(wt[..., :cv]), (n, h, w, cc), cb, cc, abs(s), stride)
    if wrong == "phase" and stride == 2:
        dx = dx.copy()
        dx[:, 1::2, 0::2] = np.roll(dx[:, 1::2, 0::2], 1, axis=2)         # one phase of the polyphase form shifted by a pixel
    if wrong == "chunk":
        drop = wt.copy()
        a, b = max(cv - 32, 0) if cv > 32 else 0, cv                      # the last k-chunk of the gradient conv: the last 32 dz channels (of its last tap)
        drop[0, 0, :, a:b] = 0.0
        dx = C.dgrad(dz, drop[..., :cv], (n, h, w, cc), cb, cc, s, stride)
    if wrong == "pad":
        dx = np.roll(dx, 1, axis=2 if w > 1 else 1)
    if wrong == "f16":
        dx = C.dgrad(C.to_f16(dz).astype(np.float64), C.to_f16(wt[..., :cv]).astype(np.float64), (n, h, w, cc), cb, cc, s, stride)
    if probe:
        return dz, wt, dx, cc
    lsb = C.common_lsb(dz) * C.common_lsb(wt[:, :, cb:cb + cc] * s)
    worst = float(total.max()) / lsb
    assert worst < LIMIT, "%s: sum |terms| / lsb = %.3g 2^24" % (o["name"], worst / LIMIT)
    assert np.array_equal(dx.astype(np.float32).astype(np.float64), dx)
    return dz, wt, dx, cc


def dgrad_wrong_models(o):
    names = ["tap", "chunk"] + (["pad"] if o["h"] * o["w"] > 1 else []) + (["phase"] if o["kind"] == "poly" and o["h"] > 1 and o["w"] > 2 else [])
    return names + (["swap"] if o["c2"] else []) + (["f16"] if o["mode"] != "int" else [])


def dgrad_kind(o):
    """dgrad_geom of conv_plan.hip under AUTO_EXACT: the fused Winograd kernel where the transposed 3x3 / 1 layer qualifies, else the MFMA /
    direct kernels; stride 2: the 1x1 coarse-grid form or the polyphase form"""
    cv = o.get("cv") or o["cout"]
    cc = o["c2"] if o["which"] else o["c1"]
    cz, ccp = -(-cv // 4) * 4, cc if cc % 16 == 0 else -(-cc // 16) * 16
    if o["stride"] == 2:
        return "1x1s2" if (o["kh"], o["kw"]) == (1, 1) else "poly"
    wino = (o["kh"], o["kw"]) == (3, 3) and cz == cv and ccp == cc and cz % 8 == 0 and cc % 64 == 0 and cz >= 32
    return "wino" if wino else "mfma"


@pytest.mark.parametrize("o", DGRAD)
def test_input_gradient(K, lib, o, monkeypatch):
    assert dgrad_kind(o) == o["kind"], (o["name"], dgrad_kind(o))
    dz, wt, dx_ref, cc = dgrad_reference(o)
    n, h, w, which = o["n"], o["h"], o["w"], o["which"]
    cv = o.get("cv") or o["cout"]
    d = K._conv_desc((n, h, w, o["c1"]), (o["kh"], o["kw"], o["c1"] + o["c2"], o["cout"]), o["stride"], o["c2"], o["x2s"], cv)
    d.algo = ALGO["exact"]
    tracks = int(lib.shdr_conv2d_dgrad_tracks_range_f32(ctypes.byref(d), which))
    assert tracks == (1 if o["kind"] == "mfma" else 0), (o["name"], tracks)
    what = "%s [%s form]" % (o["name"], o["kind"])
    nbytes = int(lib.shdr_conv2d_dgrad_workspace_bytes_f32(ctypes.byref(d), which))
    assert nbytes > 0 and nbytes % 16 == 0
    ws = Out((nbytes // 4,))                                              # exactly the bytes asked for, between guards
    dzd, wd = dev(dz), dev(wt)
    dx = Out((n, h, w, cc))
    slot = Slot((seed_of(o["name"]) % 3 == 0) * 1.0e6)
    st = K._stream()
    if not tracks:                                                        # the documented refusal of a slot the plan cannot fill; nothing written
        rc = lib.shdr_conv2d_dgrad_ranged_f32(ctypes.byref(d), which, P(dzd), P(wd), dx.ptr, ws.ptr, None, P(slot.view), st)
        assert rc == E_SHAPE, (what, rc)
        untouched(dx.buf, what + " (refused dx_range)")
        slot.check(0.0, what + " (refused dx_range)")
    rc = lib.shdr_conv2d_dgrad_ranged_f32(ctypes.byref(d), which, P(dzd), P(wd), dx.ptr, ws.ptr, None, P(slot.view) if tracks else None, st)
    assert rc == 0, (what, rc, lib.shdr_last_error())
    ws.words(what + " workspace")
    same_in_tiles(dx.words(what + " dx").view(np.float32), dx_ref, what + " dx", (8, 16))
    if tracks:
        slot.check(float(np.abs(dx_ref).max()), what)
    if o["kind"] == "1x1s2":
        got = dx.words(what).view(np.float32).copy()
        got[:, ::2, ::2] = 0.0
        assert not got.any() and not (got.view(np.uint32) != 0).any(), what + ": dx off the coarse grid must be exactly +0"


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: argument checks only (every pointer handed over is a valid, large-enough buffer); the documented code, nothing written
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(K, lib):
    n, h, w, c, cout = 1, 8, 10, 16, 16
    big = torch.zeros((1 << 16,), device="cuda")
    y, yp = Out((1 << 14,)), Out((1 << 12,))
    slot = Slot(0.0)
    R, st = P(slot.view), K._stream()

    def desc(c1=c, c2=0, co=cout, k=3, stride=1, algo="exact", **kw):
        cv = kw.pop("cv", None)
        d = K._conv_desc((n, h, w, c1), (k, k, c1 + c2, co), stride, c2, kw.pop("x2s", 1.0), cv)
        d.algo = ALGO[algo]
        for f, v in kw.items():
            setattr(d, f, v)
        return d

    def refused(rc, code, what):
        assert rc == code, (what, rc, code, lib.shdr_last_error())
        untouched(y.buf, what)
        untouched(yp.buf, what)
        slot.check(0.0, what)

    fwd = lib.shdr_conv2d_fwd_yrange_f32
    B = P(big)
    refused(fwd(ctypes.byref(desc()), B, B, B, None, None, None, None, y.ptr, R, st), E_NULL, "x2 without C2")
    refused(fwd(ctypes.byref(desc(c2=16)), B, None, B, None, None, None, None, y.ptr, R, st), E_NULL, "C2 without x2")
    refused(fwd(ctypes.byref(desc()), B, None, B, None, B, None, None, y.ptr, R, st), E_NULL, "scale without shift")
    refused(fwd(ctypes.byref(desc()), B, None, B, None, None, B, None, y.ptr, R, st), E_NULL, "shift without scale")
    refused(fwd(ctypes.byref(desc()), B, None, B, None, None, None, None, None, R, st), E_NULL, "no y")
    refused(fwd(ctypes.byref(desc(pad_t=3)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "pad_t >= KH")
    refused(fwd(ctypes.byref(desc(pad_l=-1)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "pad_l < 0")
    refused(fwd(ctypes.byref(desc(Ho=h + 2)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "Ho beyond the padded input")
    refused(fwd(ctypes.byref(desc(cv=cout + 1)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "cout_valid > Cout")
    refused(fwd(ctypes.byref(desc(y_cstride=cout - 4)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "y_cstride < stored channels")
    refused(fwd(ctypes.byref(desc(res_cstride=cout - 4)), B, None, B, None, None, None, B, y.ptr, R, st), E_SHAPE, "res_cstride < stored channels")
    refused(fwd(ctypes.byref(desc(H=0)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "H = 0")
    refused(fwd(ctypes.byref(desc(w_batch_stride=-1)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "negative w_batch_stride")
    refused(fwd(ctypes.byref(desc(y_pix_stride=2, y_H=2 * h - 2, y_W=2 * w)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "strided y too small")
    refused(fwd(ctypes.byref(desc(y_pix_stride=2, y_H=2 * h, y_W=2 * w, y_off_w=2)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "offset off the y tensor")
    d99 = desc()
    d99.algo = 99
    refused(fwd(ctypes.byref(d99), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "unknown algo")
    # a forced MFMA path on operands it cannot take
    for algo in ("mfma", "reg", "f16", "bf16"):
        refused(fwd(ctypes.byref(desc(c1=6, algo=algo)), B, None, B, None, None, None, None, y.ptr, R, st), E_ALIGN, algo + ": C1 % 4")
        refused(fwd(ctypes.byref(desc(co=24, algo=algo)), B, None, B, None, None, None, None, y.ptr, R, st), E_ALIGN, algo + ": Cout % 16")
        refused(fwd(ctypes.byref(desc(algo=algo)), P(big, 4), None, B, None, None, None, None, y.ptr, R, st), E_ALIGN, algo + ": x1 misaligned")
        refused(fwd(ctypes.byref(desc(algo=algo)), B, None, P(big, 8), None, None, None, None, y.ptr, R, st), E_ALIGN, algo + ": w misaligned")
        refused(fwd(ctypes.byref(desc(algo=algo)), B, None, B, P(big, 4), None, None, None, y.ptr, R, st), E_ALIGN, algo + ": bias misaligned")
        refused(fwd(ctypes.byref(desc(algo=algo, y_cstride=cout + 2)), B, None, B, None, None, None, None, y.ptr, R, st), E_ALIGN, algo + ": y_cstride % 4")
        refused(fwd(ctypes.byref(desc(algo=algo, res_cstride=cout + 2)), B, None, B, None, None, None, B, y.ptr, R, st), E_ALIGN, algo + ": res_cstride % 4")
    for algo in ("f16", "bf16"):
        refused(fwd(ctypes.byref(desc(c2=16, algo=algo, x2s=0.5)), B, B, B, None, None, None, None, y.ptr, R, st), E_SHAPE, algo + ": x2_scale != 1")
    # the direct path: padded filters, per-image filters, a range slot of a strided or channel-padded output
    refused(fwd(ctypes.byref(desc(algo="direct", cv=3)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "direct: padded filter")
    refused(fwd(ctypes.byref(desc(algo="direct", w_batch_stride=9 * c * cout)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "direct: per-image filters")
    refused(fwd(ctypes.byref(desc(c1=6, y_cstride=cout + 1)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE, "direct: y_range of a channel-padded y")
    refused(fwd(ctypes.byref(desc(c1=6, y_pix_stride=2, y_H=2 * h, y_W=2 * w)), B, None, B, None, None, None, None, y.ptr, R, st), E_SHAPE,
            "direct: y_range of a strided y")
    # the fused Winograd entry points
    f2, fu = lib.shdr_conv2d_winograd_fused2_f32, lib.shdr_conv2d_winograd_fused_up2_f32
    refused(f2(B, None, B, None, None, None, y.ptr, yp.ptr, 1, 7, 8, 32, 0, 64, 0, 0, st), E_SHAPE, "fused: pooled output of an odd H")
    refused(f2(B, None, B, None, None, None, None, None, 1, 8, 8, 32, 0, 64, 0, 0, st), E_NULL, "fused: neither y nor y_pool")
    refused(f2(B, B, B, None, None, None, y.ptr, None, 1, 8, 8, 32, 0, 64, 0, 0, st), E_NULL, "fused: x2 without C2")
    refused(f2(B, B, B, None, None, None, y.ptr, None, 1, 8, 8, 32, 16, 64, 0, 0, st), E_SHAPE, "fused: C2 != C1")
    refused(f2(B, None, B, None, B, None, y.ptr, None, 1, 8, 8, 32, 0, 64, 0, 0, st), E_NULL, "fused: scale without shift")
    refused(f2(B, None, B, None, None, None, y.ptr, None, 1, 8, 8, 12, 0, 64, 0, 0, st), E_SHAPE, "fused: Cin % 8")
    refused(f2(B, None, B, None, None, None, y.ptr, None, 1, 8, 8, 32, 0, 48, 0, 0, st), E_SHAPE, "fused: Cout % 64")
    refused(f2(P(big, 4), None, B, None, None, None, y.ptr, None, 1, 8, 8, 32, 0, 64, 0, 0, st), E_ALIGN, "fused: x misaligned")
    refused(fu(B, B, None, None, None, y.ptr, 1, 7, 8, 32, 64, 0, 0, st), E_SHAPE, "fused up2: odd H")
    refused(fu(B, B, None, None, None, None, 1, 8, 8, 32, 64, 0, 0, st), E_NULL, "fused up2: no y")
    refused(fu(B, P(big, 8), None, None, None, y.ptr, 1, 8, 8, 32, 64, 0, 0, st), E_ALIGN, "fused up2: u misaligned")
    # the transform kernels
    refused(lib.shdr_winograd_input_f32(B, y.ptr, 1, 8, 8, 6, st), E_SHAPE, "winograd_input: C % 4")
    refused(lib.shdr_winograd_input_f32(P(big, 4), y.ptr, 1, 8, 8, 8, st), E_ALIGN, "winograd_input: x misaligned")
    refused(lib.shdr_winograd_output_f32(B, y.ptr, None, B, None, 1, 8, 8, 8, 0, 0, st), E_NULL, "winograd_output: scale without shift")
    refused(lib.shdr_winograd_output_f32(B, y.ptr, None, None, None, 1, 8, 8, 6, 0, 0, st), E_SHAPE, "winograd_output: C % 4")
    refused(lib.shdr_winograd_filter_packed_f32(B, y.ptr, 12, 64, st), E_SHAPE, "winograd_filter_packed: Cin % 8")
    refused(lib.shdr_winograd_filter_f32(B, y.ptr, 0, 64, st), E_SHAPE, "winograd_filter: Cin = 0")
    # the input gradient
    dg = lib.shdr_conv2d_dgrad_ranged_f32
    refused(dg(ctypes.byref(desc()), 1, B, B, y.ptr, B, None, None, st), E_SHAPE, "dgrad: which = 1 without C2")
    refused(dg(ctypes.byref(desc(stride=3)), 0, B, B, y.ptr, B, None, None, st), E_SHAPE, "dgrad: stride 3")
    refused(dg(ctypes.byref(desc(k=2)), 0, B, B, y.ptr, B, None, None, st), E_SHAPE, "dgrad: even filter at stride 1")
    refused(dg(ctypes.byref(desc()), 0, B, B, y.ptr, None, None, None, st), E_NULL, "dgrad: no workspace")
    refused(dg(ctypes.byref(desc()), 0, P(big, 4), B, y.ptr, B, None, None, st), E_ALIGN, "dgrad: dz misaligned")
    refused(dg(ctypes.byref(desc(stride=2)), 0, B, B, y.ptr, B, None, R, st), E_SHAPE, "dgrad: dx_range at stride 2")
    assert int(lib.shdr_conv2d_dgrad_workspace_bytes_f32(ctypes.byref(desc()), 1)) == -1 and int(lib.shdr_conv2d_dgrad_tracks_range_f32(ctypes.byref(desc()), 1)) == 0
