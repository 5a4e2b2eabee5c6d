"""The camera-simulator kernels (csrc/camera.hip) element by element and byte by byte, at the qualities, inputs,
thresholds and sizes that tests/test_gpu_camera.py leaves out.  The inputs live in tests/camera_ref.py; tests/test_camera.py shows on
the CPU that a kernel with a wrong rounding, quality scale, table, up-sampling, threshold or noise term would fail AT THESE INPUTS.

jpeg_round_trip: bytes against oracle.camera.jpeg_round_trip and against libjpeg itself (Pillow), at qualities 1 .. 100 with several
in one batch, on inputs OFF the 8-bit grid (below 0, above 1, every tie x * 255 = k + 0.5: expected byte clip(rint(fl32(x * 255)), 0,
255), half to even), at one MCU (the fancy up-sampling meets all four image edges) and at 528 x 512 = 270336 pixels, more than the
finish kernel's 1024 x 256 threads.  The loss mask is tested AT its thresholds: exactly 32768 pixels at grey 249 / 6 keep the sample,
32769 drop it.

camera_expose: |got - ref| <= K_EXPOSE u scale PER ELEMENT against camera_ref.expose64, u = 2^-24, scale = |x| + (sigma_s |x| +
sigma_c) rad.  K_EXPOSE comes from a measurement against the float64 reference, not from the oracle or the kernel's own output: the
worst err / (u scale) of the device over the four cases is 3.256 (at 2 x 300 x 300; the fp32 numpy restatement alone: 3.6), and
K_EXPOSE = 13.1 is four times the device's figure -- the margin is for logf / cosf / sinf, whose last place differs between libraries.  K_EXPOSE <= 32 is what
keeps the bound from hiding a fault: the wrong models of tests/test_camera.py miss it by orders of magnitude."""
import io

import numpy as np
import pytest
import torch

import camera_ref as R
from oracle import camera as O
from test_gpu_wgrad_f32_exact import P, guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

E_SHAPE, E_NULL = -1, -5


@pytest.fixture(scope="module")
def lib(shdr):
    return shdr._lib.load()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def pil_round_trip(img, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=q, subsampling=2)
    return np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


class Workspace:
    def __init__(self, n, h, w):
        self.planes = torch.empty(n * h * w * 3 // 2, device="cuda", dtype=torch.uint8)
        self.counts = torch.full((2 * n,), 12345, device="cuda", dtype=torch.int32)          # the call must zero them itself


def round_trip(lib, ldr, quality, ws=None, want_mask=True):
    """(bytes uint8 [N, H, W, 3], mask [N] or None) through the C ABI, outputs between guard words; the float output is checked to
    be u8 / 255 IN BITS"""
    n, h, w, _ = ldr.shape
    ws = ws or Workspace(n, h, w)
    jbuf, jview = guarded(ldr.size)
    mbuf, mview = guarded(n)
    x, q = dev(ldr.astype(np.float32)), dev(np.asarray(quality, dtype=np.int32))
    jf = jview.view(torch.float32)
    rc = lib.shdr_jpeg_round_trip_f32(P(x), P(q), P(jf), P(mview) if want_mask else None, P(ws.planes), P(ws.counts), n, h, w, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    guards_intact(jbuf, ldr.size, "jpeg")
    got = jf.cpu().numpy().reshape(ldr.shape)
    u8 = np.rint(got * np.float32(255)).astype(np.uint8)
    assert np.array_equal(got.view(np.uint32), (u8.astype(np.float32) / np.float32(255)).view(np.uint32)), "jpeg is not u8 / 255 in bits"
    if not want_mask:
        untouched(mbuf, "loss_mask == NULL")
        return u8, None
    guards_intact(mbuf, n, "loss_mask")
    return u8, mview.view(torch.float32).cpu().numpy()


def same_bytes(got, want, what):
    bad = got != want
    if bad.any():
        i = tuple(int(v) for v in np.unravel_index(int(np.argmax(bad)), bad.shape))
        raise AssertionError("%s: %d of %d bytes differ; first at %s: got %d, want %d" % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


# ---------------------------------------------------------------------------------------------------------------------------------
# jpeg_round_trip
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.JPEG_SIZES, ids=lambda s: "%dx%d" % s)
def test_jpeg_round_trip_bytes(lib, size):
    h, w = size
    even = {k % 2 for _, k in R.ties()}
    assert even == {0, 1}, "ties with even and with odd k must both be present"
    for ldr, q in R.jpeg_batches(h, w):
        assert len({ldr[i].tobytes() for i in range(3)}) == 3 and len(set(q)) == 3
        got, mask = round_trip(lib, ldr, q)
        for i in range(3):
            what = "jpeg %dx%d sample %d quality %d" % (h, w, i, q[i])
            u8 = R.quantise_u8(ldr[i])
            same_bytes(got[i], O.jpeg_round_trip(u8, q[i]), what + " vs oracle")
            same_bytes(got[i], pil_round_trip(u8, q[i]), what + " vs libjpeg")
        assert mask.tolist() == [float(O.loss_mask(got[i:i + 1]).reshape(())) for i in range(3)]


def test_jpeg_quality_is_clamped_to_1_100(lib):
    ldr = np.stack([R.jpeg_contents(16, 48, s)["noise"] for s in range(3)])
    for given, means in R.JPEG_CLAMPED:
        got, _ = round_trip(lib, ldr, given)
        want, _ = round_trip(lib, ldr, means)
        same_bytes(got, want, "quality %s vs %s" % (given, means))
        for i in range(3):
            same_bytes(got[i], O.jpeg_round_trip(R.quantise_u8(ldr[i]), means[i]), "quality %d vs oracle at %d" % (given[i], means[i]))


# ---------------------------------------------------------------------------------------------------------------------------------
# loss mask at its thresholds
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.mask_cases()))
def test_loss_mask_thresholds(lib, name):
    img, counts, want = R.mask_cases()[name]
    assert R.census(O.jpeg_round_trip(img, 100)) == counts, "precondition: the oracle's census of this input"
    assert R.loss_mask(O.jpeg_round_trip(img, 100)) == want
    other = np.full_like(img, 128)                                       # a neighbour whose counts must not leak: kept
    batch = np.stack([other, img, other]).astype(np.float32) / np.float32(255)
    ws = Workspace(*batch.shape[:3])
    got, mask = round_trip(lib, batch, [100, 100, 100], ws)
    same_bytes(got[1], O.jpeg_round_trip(img, 100), name)
    assert mask.tolist() == [1.0, want, 1.0], (name, mask.tolist(), ws.counts.tolist())
    assert ws.counts.tolist()[2:4] == list(counts), "the device's census"
    again, mask2 = round_trip(lib, batch, [100, 100, 100], ws)           # the same workspace: the counts are zeroed by the call
    assert mask2.tolist() == mask.tolist() and np.array_equal(again, got) and ws.counts.tolist()[2:4] == list(counts)
    same, none = round_trip(lib, batch, [100, 100, 100], ws, want_mask=False)
    assert none is None and np.array_equal(same, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# camera_expose
# ---------------------------------------------------------------------------------------------------------------------------------
def expose(lib, hdr, t, seed, what="camera_expose"):
    n, h, w, _ = hdr.shape
    tb, tv = guarded(hdr.size)
    cb, cv = guarded(hdr.size)
    x, td = dev(hdr), dev(t)
    a, b = tv.view(torch.float32), cv.view(torch.float32)
    assert lib.shdr_camera_expose_f32(P(x), P(td), P(a), P(b), n, h, w, seed, None) == 0, what
    torch.cuda.synchronize()
    guards_intact(tb, hdr.size, what + " hdr_t")
    guards_intact(cb, hdr.size, what + " clipped")
    return a.cpu().numpy().reshape(hdr.shape), b.cpu().numpy().reshape(hdr.shape)


@pytest.mark.parametrize("case", R.EXPOSE_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_camera_expose_per_element(lib, case):
    assert R.K_EXPOSE <= 32
    hdr, t, seed = R.expose_input(case)
    want, _, scale = R.expose64(hdr, t, seed)
    got, clipped = expose(lib, hdr, t, seed)
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / (R.U * np.maximum(scale, 1e-300))
    i = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    print("camera_expose %s: worst err / (u scale) = %.3f at %s (got %r, want %r)" % (case, ratio[i], i, float(got[i]), float(want[i])))
    assert np.all(err <= R.K_EXPOSE * R.U * scale), (case, i, float(ratio[i]))
    assert np.array_equal(clipped.view(np.uint32), np.minimum(got, np.float32(1)).view(np.uint32)) and got.min() >= 0
    zero = (hdr * t.reshape(-1, 1, 1, 1)) == 0                           # v = max(sigma_c z1, 0): about half of these are noise
    if zero.sum() > 1000:
        assert 0.3 < (got[zero] > 0).mean() < 0.7
    again, _ = expose(lib, hdr, t, seed)
    other, _ = expose(lib, hdr, t, seed + 1)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and not np.array_equal(other, got)


def test_camera_expose_does_not_depend_on_the_batch_cut(lib):
    hdr, t, seed = R.expose_input((3, 40, 56))
    full, _ = expose(lib, hdr, t, seed)
    two, _ = expose(lib, hdr[:2], t[:2], seed)
    assert np.array_equal(full[:2].view(np.uint32), two.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(lib):
    x = dev(np.full(2 * 32 * 32 * 3, 0.5, dtype=np.float32))
    q = dev(np.array([90, 90], dtype=np.int32))
    t = dev(np.ones(2, dtype=np.float32))
    ws = Workspace(2, 32, 32)
    buf, view = guarded(2 * 32 * 32 * 3)
    y = view.view(torch.float32)
    mbuf, mview = guarded(2)

    def jpeg(n, h, w, ldr=x, qual=q, out=y, planes=ws.planes, counts=ws.counts):
        return lib.shdr_jpeg_round_trip_f32(P(ldr), P(qual), P(out), P(mview), P(planes), P(counts), n, h, w, None)
    calls = {
        "jpeg N = 0": (E_SHAPE, lambda: jpeg(0, 32, 32)), "jpeg N < 0": (E_SHAPE, lambda: jpeg(-1, 32, 32)),
        "jpeg H = 0": (E_SHAPE, lambda: jpeg(2, 0, 32)), "jpeg W = 0": (E_SHAPE, lambda: jpeg(2, 32, 0)),
        "jpeg H < 0": (E_SHAPE, lambda: jpeg(2, -16, 32)), "jpeg W < 0": (E_SHAPE, lambda: jpeg(2, 32, -16)),
        "jpeg H % 16": (E_SHAPE, lambda: jpeg(2, 24, 32)), "jpeg W % 16": (E_SHAPE, lambda: jpeg(2, 32, 24)),
        "jpeg N > 65535": (E_SHAPE, lambda: jpeg(65536, 16, 16)),
        "jpeg null ldr": (E_NULL, lambda: jpeg(2, 32, 32, ldr=None)), "jpeg null quality": (E_NULL, lambda: jpeg(2, 32, 32, qual=None)),
        "jpeg null planes": (E_NULL, lambda: jpeg(2, 32, 32, planes=None)),
        "jpeg null counts": (E_NULL, lambda: jpeg(2, 32, 32, counts=None)),
        "expose N = 0": (E_SHAPE, lambda: lib.shdr_camera_expose_f32(P(x), P(t), P(y), P(y), 0, 32, 32, 1, None)),
        "expose H = 0": (E_SHAPE, lambda: lib.shdr_camera_expose_f32(P(x), P(t), P(y), P(y), 2, 0, 32, 1, None)),
        "expose W < 0": (E_SHAPE, lambda: lib.shdr_camera_expose_f32(P(x), P(t), P(y), P(y), 2, 32, -1, 1, None)),
        "expose null hdr": (E_NULL, lambda: lib.shdr_camera_expose_f32(None, P(t), P(y), P(y), 2, 32, 32, 1, None)),
        "expose null t": (E_NULL, lambda: lib.shdr_camera_expose_f32(P(x), None, P(y), P(y), 2, 32, 32, 1, None)),
        "expose null clipped": (E_NULL, lambda: lib.shdr_camera_expose_f32(P(x), P(t), P(y), None, 2, 32, 32, 1, None)),
    }
    for what, (code, call) in calls.items():
        assert call() == code, what
        untouched(buf, what)
        untouched(mbuf, what)
    assert jpeg(2, 32, 32, out=None) == E_NULL
    assert lib.shdr_camera_expose_f32(P(x), P(t), None, P(y), 2, 32, 32, 1, None) == E_NULL
    untouched(buf, "expose null hdr_t")
