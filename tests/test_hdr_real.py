"""HDR-Real folder reader, host side (singlehdr-tf2_amd/hdr_real.py): the patch enumeration of convert_to_tf_record.py:71-86 with its
quirks, the order of the grey value at the filter's thresholds, and the converter's file naming and split.  No GPU is needed."""
import glob
import os

import numpy as np

import hdr_real_ref as R


def test_one_patch_when_the_image_is_the_patch(shdr):
    assert shdr.hdr_real.enumerate_patches(256, 256) == [(0, 0)]


def test_no_patch_when_a_side_is_smaller_than_the_patch(shdr):
    assert shdr.hdr_real.enumerate_patches(255, 300) == []
    assert shdr.hdr_real.enumerate_patches(300, 255) == []


def test_multiple_of_the_patch_has_the_grid_only(shdr):
    grid = [(h, w) for h in (0, 64, 128, 192, 256) for w in (0, 64, 128, 192, 256)]
    assert shdr.hdr_real.enumerate_patches(512, 512) == grid and len(grid) == 25


def test_border_row_is_written_twice_when_the_grid_already_reaches_it(shdr):
    """the border tests are `% size`, not `% stride`: h = 320 gives row 64 from the grid and again as the border row"""
    assert shdr.hdr_real.enumerate_patches(320, 256) == [(0, 0), (64, 0), (64, 0)]


def test_grid_then_bottom_row_then_right_column_then_corner(shdr):
    want = [(0, 0), (0, 64),                 # grid: rows range(0, 45, 64), columns range(0, 78, 64)
            (44, 0), (44, 64),               # 300 % 256: bottom row at 300 - 256
            (0, 77),                         # 333 % 256: right column at 333 - 256
            (44, 77)]                        # both: the corner
    assert shdr.hdr_real.enumerate_patches(300, 333) == want


def test_small_size_and_stride(shdr):
    want = [(0, 0), (0, 4), (4, 0), (4, 4),  # 22 x 23, size 16, stride 4: rows 0, 4 and columns 0, 4
            (6, 0), (6, 4),                  # 22 % 16: bottom row at 6
            (0, 7), (4, 7),                  # 23 % 16: right column at 7
            (6, 7)]
    assert shdr.hdr_real.enumerate_patches(22, 23, size=16, stride=4) == want


def test_grey_order_census_over_all_8_bit_triples(shdr):
    """A finding, not a gate: over all 256^3 (r, g, b) the extreme predicate (grey >= 249 or <= 6) is compared between the
    specified order (fp32, left to right, unfused), a fully fused evaluation and the reversed order; the counts are in DESIGN.md
    and say how many pixel values could ever flip a keep / drop decision against cv2, whose order was not checked.  Asserted: the
    restatement the GPU tests use IS the specified order, each step emulated here as an exact float64 operation rounded to fp32."""
    v = np.arange(256)
    r, g, b = v[:, None, None], v[None, :, None], v[None, None, :]
    f64 = np.float64
    pr, pg, pb = ((c.astype(f64) * f64(k)).astype(np.float32) for c, k in ((r, R.CR), (g, R.CG), (b, R.CB)))       # products: exact in float64
    spec = ((pr.astype(f64) + pg.astype(f64)).astype(np.float32).astype(f64) + pb.astype(f64)).astype(np.float32)  # sums: exact in float64
    ref = R.gray(*np.broadcast_arrays(r, g, b))
    assert spec.shape == (256, 256, 256) and np.array_equal(spec, ref)
    e_spec = R.extreme(spec)
    e_fused = R.extreme(R.gray_fused(*np.broadcast_arrays(r, g, b)))
    e_rev = R.extreme(R.gray_reversed(*np.broadcast_arrays(r, g, b)))
    print("grey census: extreme under the specified order %d; differs when fused %d; differs when reversed %d; fused vs reversed %d"
          % (int(e_spec.sum()), int((e_spec != e_fused).sum()), int((e_spec != e_rev).sum()), int((e_fused != e_rev).sum())))
    # the product's host helper is the same order
    px = np.stack(np.broadcast_arrays(r, g, b), -1)[::5, ::3, ::7].astype(np.uint8)
    assert shdr.hdr_real.extreme_pixels(px) == int(e_spec[::5, ::3, ::7].sum())


class _FakeFolder:
    """what write_tfrecords needs of a folder: 70 kept 4 x 4 patches of one 4 x 280 pair, on the host"""
    size, stride = 4, 4

    def __init__(self):
        rng = np.random.default_rng(0)
        self.ldr = rng.integers(0, 256, (4, 280, 3), dtype=np.uint8)
        self.hdr = rng.random((4, 280, 3), dtype=np.float32) * 8
        self.patches = [(0, 0, 4 * k) for k in range(70)]

    def host_pair(self, f):
        assert f == 0
        return self.ldr, self.hdr


def test_write_tfrecords_names_and_32_per_file(shdr, tmp_path):
    folder = _FakeFolder()
    paths = shdr.hdr_real.write_tfrecords(folder, str(tmp_path / "rec"))
    assert [os.path.basename(p) for p in paths] == ["train_4_0000.tfrecords", "train_4_0001.tfrecords", "train_4_0002.tfrecords"]
    assert sorted(glob.glob(str(tmp_path / "rec" / "*"))) == paths
    T = shdr.tfrecord
    k = 0
    for path, n in zip(paths, (32, 32, 6)):
        recs = list(T.read_records(path))
        assert len(recs) == n
        for rec in recs:
            ex = T.parse_example(rec)
            assert sorted(ex) == ["ref_HDR", "ref_LDR"]
            hdr = np.frombuffer(ex["ref_HDR"][0], dtype="<f4").reshape(4, 4, 3)
            ldr = np.frombuffer(ex["ref_LDR"][0], dtype="<f4").reshape(4, 4, 3)
            assert np.array_equal(hdr, folder.hdr[:, 4 * k:4 * k + 4])               # raw HDR values
            assert np.array_equal(ldr, folder.ldr[:, 4 * k:4 * k + 4].astype(np.float32))         # LDR 0 .. 255 as float32
            k += 1
    assert k == 70
    again = shdr.hdr_real.write_tfrecords(folder, str(tmp_path / "rec7"), records_per_file=7)
    assert len(again) == 10 and os.path.basename(again[-1]) == "train_4_0009.tfrecords"
