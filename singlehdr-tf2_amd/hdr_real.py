"""Fine-tuning from HDR-Real image folders: the pairs live on the device, a batch is one launch.

    folder = HdrRealFolder("HDR-Real")                       # HDR-Real/HDR_gt/*.hdr + HDR-Real/LDR_in/*.jpg
    for ref_LDR, ref_HDR in folder:                          # float32 [b, 256, 256, 3] on the device, one epoch
        step(ref_LDR, ref_HDR)                               # pipeline.FinetuneStep
    write_tfrecords(folder, "tf_records/256_64_b32_tfrecords")          # the reference's records, for tfrecord.HdrRealDataset

The reference gets here in two steps.  convert_to_tf_record.py cuts every pair into 256 x 256 patches at stride 64, drops the
patches that are mostly black or white and stores the rest as float32 in GZIP TFRecords (each pixel about 16 times, 24 B per
pixel pair); finetune_real_dataset.py:34-78 reads them back, normalises the HDR patch to mean 0.5, divides the LDR patch by 255
and applies a random flip and rot90.  Here every pair is read once: the LDR image stays uint8 RGB (3 B / pixel) and the HDR image
float32 RGB in two flat device arenas that share one offset table (as dataset.PatchHDRDataset keeps its files).  One launch of the
statistics kernel computes the filter's extreme-pixel count and the mean of every candidate patch; a batch is one launch of the
gather kernel (csrc/hdr_real.hip), which crops, flips, rotates and normalises both patches of every sample.

Who checks the tables: libshdr.  The kernels index the arenas with the image / patch / sample tables and trust them; the launchers
(include/shdr.h) take every table as a host array, validate it and only then launch on the device copy this module made from
that very array.  A bad table never launches.

Channel order is the records': RGB (cv2's BGR is reversed at convert_to_tf_record.py:50-51).  cv2 is not a dependency: the JPEG
decoder is PIL's (hdr_io.read_ldr), Radiance files are Ward's RGBE decode without the +0.5 (as cv2.imread), OpenEXR files as exr.py
reads them, unclipped.  The grey value of the filter is r*0.299f + g*0.587f + b*0.114f in fp32, left to right, unfused; cv2's own
order was never run here (DESIGN.md has the census of values at which the orders disagree).
"""
import glob
import os
import time

import numpy as np
import torch

try:
    from . import _ops as K
    from . import exr
    from . import hdr_io
    from . import jpeg
    from . import tfrecord
except ImportError:
    import _ops as K
    import exr
    import hdr_io
    import jpeg
    import tfrecord

SIZE = 256                     # patch_size   (convert_to_tf_record.py:12)
STRIDE = 64                    # patch_stride (:13)
RECORDS_PER_FILE = 32          # batch_size   (:14): records per .tfrecords file
BATCH_SIZE = tfrecord.BATCH_SIZE
GRAY_HI, GRAY_LO = 249.0, 6.0  # :55

S_PATCH, S_FLIP, S_ROT = range(3)          # columns of the sample table of draw() / render()


def enumerate_patches(h, w, size=SIZE, stride=STRIDE):
    """the (h1, w1) corners convert_to_tf_record.py:71-86 visits on an h x w image, in its order: the regular grid, the bottom
    row if h % size, the right column if w % size, the corner if both.  The border tests are `% size`, not `% stride`, so a border
    patch that the grid already holds is listed (and written) twice, e.g. row 64 of a 320 x 256 image.  An image smaller than
    `size` on either side has no patch (the reference's negative slice start would cut a sliver; it is not reproduced)."""
    h, w, size, stride = int(h), int(w), int(size), int(stride)
    if size <= 0 or stride <= 0:
        raise ValueError("enumerate_patches: size and stride must be positive")
    if h < size or w < size:
        return []
    rows, cols = range(0, h - size + 1, stride), range(0, w - size + 1, stride)
    out = [(h_, w_) for h_ in rows for w_ in cols]
    if h % size:
        out += [(h - size, w_) for w_ in cols]
    if w % size:
        out += [(h_, w - size) for h_ in rows]
    if w % size and h % size:
        out.append((h - size, w - size))
    return out


def extreme_pixels(ldr_patch):
    """the count of convert_to_tf_record.py:54-55 on a uint8 RGB patch, host NumPy: fp32, left to right, every step rounded"""
    p = np.asarray(ldr_patch).astype(np.float32)
    gray = (p[..., 0] * np.float32(0.299) + p[..., 1] * np.float32(0.587)) + p[..., 2] * np.float32(0.114)
    return int(np.sum(gray >= np.float32(GRAY_HI)) + np.sum(gray <= np.float32(GRAY_LO)))


class HdrRealFolder:
    """The HDR-Real pairs of `dirpath` on the device, and batches of (ref_LDR, ref_HDR) as finetune_real_dataset.py's
    configureDataset yields them.

    patches          the kept patches [(file, h1, w1), ...] in the reference's writing order, duplicates included
    candidates       every patch enumerate_patches lists, kept or not, in the same order
    extreme_counts   int32 per candidate: pixels with grey >= 249 or <= 6; a candidate is kept when count <= size*size // 2
    means            float32 per candidate: the HDR patch mean, summed in float64
    keep             bool per candidate
    draw(b)          the next b samples of this rank: int32 [b, 3] (index into `patches`, flip, rot), host
    render(params)   (ref_LDR, ref_HDR) float32 [b, size, size, 3] on the device for such a table: one launch
    iter(folder)     one epoch: a seeded permutation of the kept patches (the same on every rank), of which rank r takes the
                     elements r::world_size, in batches of batch_size (the last one may be short: drop_remainder=False)
    Flips are u0 < 0.5 and rots int(u1 * 4 + 0.5) of float32 uniforms, as tfrecord.HdrRealDataset draws them: rot 4 occurs and is
    rot 0.  augment=False gives flip 0 and rot 0.
    jpeg_decoder="device" decodes all LDR files in ONE jpeg.decode batch whose output arena IS ldr_arena (the same bytes as "pil",
    hdr_io.read_ldr; files outside the device decoder's scope are read by PIL, the others still in one batch); "device_scan" is the
    same with the scans prepared on the device too (jpeg.Decoded(unstuff="device")).
    exr_inflate="device" leaves the ZIP / ZIPS chunks of OpenEXR files to the device (exr.read_stored, then ONE exr.upload_batch for
    all of them; the same arena as with "host", where zlib inflates them one file after the other).
    exr_piz: PIZ-compressed OpenEXR files are refused ("refuse", the default), decoded by libshdr's host routine ("host") or on the
    device in that one batch ("device", K.piz_decode); the arena is the same either way.
    hdr_rle="device" decodes the scanlines of all Radiance files in ONE hdr_io.rle_decode_device (the coded bytes are uploaded, not
    4 B / pixel per file); "host" (the default) runs shdr_rgbe_rle_decode file by file; the arena is the same."""

    def __init__(self, dirpath, device=None, size=SIZE, stride=STRIDE, seed=0, rank=0, world_size=1, batch_size=BATCH_SIZE,
                 augment=True, jpeg_decoder="pil", exr_inflate="host", exr_piz="refuse", hdr_rle="host"):
        if jpeg_decoder not in ("pil", "device", "device_scan"):
            raise ValueError("HdrRealFolder: jpeg_decoder must be 'pil', 'device' or 'device_scan', got %r" % (jpeg_decoder,))
        exr.check_inflate_option("HdrRealFolder", exr_inflate)
        exr.check_piz_option("HdrRealFolder", exr_piz)
        hdr_io.check_decoder_option("HdrRealFolder", hdr_rle)
        hdr_paths = sorted(p for ext in ("*.hdr", "*.exr") for p in glob.glob(os.path.join(dirpath, "HDR_gt", ext)))
        ldr_paths = sorted(glob.glob(os.path.join(dirpath, "LDR_in", "*.jpg")))
        if len(hdr_paths) != len(ldr_paths):
            raise ValueError("HdrRealFolder: %d HDR files but %d LDR files under %s: %s / %s" % (
                len(hdr_paths), len(ldr_paths), dirpath, hdr_paths, ldr_paths))
        if not hdr_paths:
            raise FileNotFoundError("HdrRealFolder: no HDR_gt/*.hdr (or *.exr) + LDR_in/*.jpg under %s" % dirpath)
        t0 = time.perf_counter()
        device = device or torch.device("cuda", torch.cuda.current_device())
        ldr_arena = None
        if jpeg_decoder != "pil":
            ldr, ldr_arena = self._decode_ldr_on_device(ldr_paths, device, "device" if jpeg_decoder == "device_scan" else "host")
        else:
            ldr = [hdr_io.read_ldr(p) for p in ldr_paths]
        read_radiance = hdr_io.read_scanlines if hdr_rle == "device" else hdr_io.read_rgbe
        hdr = [exr.read_item(p, exr_inflate, exr_piz) if exr.is_exr(p) else read_radiance(p) for p in hdr_paths]
        self.files = list(zip(hdr_paths, ldr_paths))
        self._setup(ldr, hdr, device, size, stride, seed, rank, world_size, batch_size, augment, time.perf_counter() - t0, ldr_arena)

    @staticmethod
    def _decode_ldr_on_device(paths, device, unstuff="host"):
        """(uint8 [H, W, 3] device views per file, the flat arena they lie in).  Every baseline JPEG of the folder is decoded in ONE
        jpeg batch; when all files are such and stored upright, the batch's output arena is returned as it is.  Files outside the
        decoder's scope (progressive, CMYK, ...) are read by PIL and uploaded, files with an EXIF Orientation are turned, and the
        arena is then assembled from the pieces: still one batch, whatever the number of files.  unstuff="device": the host looks at
        the headers only; a file that turns out of scope in its scan (fill bytes, a second scan) is named by the batch call, left to
        PIL, and the batch is called again without it."""
        in_scope = []
        for i, p in enumerate(paths):
            try:
                with open(p, "rb") as f:
                    jpeg.device_tables((jpeg.parse_header if unstuff == "device" else jpeg.parse)(f.read()))
                in_scope.append(i)
            except jpeg.Unsupported:
                pass
        images = [None] * len(paths)
        d = None
        while in_scope and d is None:
            try:
                d = jpeg.Decoded([paths[i] for i in in_scope], device, unstuff=unstuff)
            except jpeg.Unsupported as exc:
                if unstuff != "device" or getattr(exc, "index", None) is None:
                    raise
                del in_scope[exc.index]
        if in_scope:
            d.check()
            if len(in_scope) == len(paths) and all(h.orientation == 1 for h in d.plan.headers):
                return [d.image(i) for i in range(len(paths))], d.out
            for k, i in enumerate(in_scope):
                images[i] = jpeg.apply_orientation(d.image(k), d.plan.headers[k].orientation)
        for i, p in enumerate(paths):
            if images[i] is None:
                images[i] = torch.from_numpy(hdr_io.read_ldr(p)).to(device)
        arena = torch.cat([a.reshape(-1) for a in images])
        sizes = np.cumsum([0] + [a.numel() for a in images])
        return [arena[sizes[i]:sizes[i + 1]].view(a.shape) for i, a in enumerate(images)], arena

    @classmethod
    def from_arrays(cls, ldr_list, hdr_list, device=None, size=SIZE, stride=STRIDE, seed=0, rank=0, world_size=1,
                    batch_size=BATCH_SIZE, augment=True):
        """the same object from images in memory: ldr_list uint8 RGB [H, W, 3], hdr_list float RGB [H, W, 3] (host arrays)"""
        ldr_list, hdr_list = list(ldr_list), list(hdr_list)
        if len(ldr_list) != len(hdr_list) or not ldr_list:
            raise ValueError("HdrRealFolder.from_arrays: %d LDR and %d HDR images" % (len(ldr_list), len(hdr_list)))
        ldr = []
        for i, a in enumerate(ldr_list):
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("HdrRealFolder.from_arrays: LDR image %d must be uint8 [H, W, 3]" % i)
            ldr.append(a)
        hdr = [np.ascontiguousarray(a, dtype=np.float32) for a in hdr_list]
        self = cls.__new__(cls)
        self.files = [("hdr[%d]" % i, "ldr[%d]" % i) for i in range(len(ldr))]
        self._setup(ldr, hdr, device, size, stride, seed, rank, world_size, batch_size, augment, 0.0)
        return self

    # --- loading ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _hdr_shape(item):
        if isinstance(item, (exr.Payload, exr.Stored)):
            return item.header.height, item.header.width
        return tuple(item.shape[:2])

    def _setup(self, ldr, hdr, device, size, stride, seed, rank, world_size, batch_size, augment, host_seconds, ldr_arena=None):
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.size, self.stride, self.batch_size, self.augment = int(size), int(stride), int(batch_size), bool(augment)
        self.rank, self.world_size = int(rank), int(world_size)
        if self.size <= 0 or self.stride <= 0 or self.batch_size <= 0 or not 0 <= self.rank < self.world_size:
            raise ValueError("HdrRealFolder: size, stride and batch_size must be positive and 0 <= rank < world_size")
        shapes = []
        for i, (l, h) in enumerate(zip(ldr, hdr)):
            hs = self._hdr_shape(h)
            if tuple(l.shape[:2]) != hs or (not isinstance(h, (exr.Payload, exr.Stored, hdr_io.Scanlines)) and h.ndim != 3):
                raise ValueError("HdrRealFolder: %s is %d x %d but %s is %d x %d" % (
                    self.files[i][0], hs[0], hs[1], self.files[i][1], l.shape[0], l.shape[1]))
            shapes.append(hs)
        t0 = time.perf_counter()
        pixels = [h * w for h, w in shapes]
        offsets = np.concatenate([[0], np.cumsum(pixels)[:-1]]).astype(np.int64)
        total = int(sum(pixels))
        self.shapes = shapes
        self.images = np.ascontiguousarray(np.column_stack([offsets, np.asarray(shapes, dtype=np.int64).reshape(-1, 2)]), dtype=np.int64)
        if ldr_arena is not None:                                  # decoded on the device, already flat in file order
            self.ldr_arena = ldr_arena
        else:
            self.ldr_arena = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in ldr])).to(self.device)
        self.hdr_arena = torch.empty(total * 3, device=self.device, dtype=torch.float32)
        batched = {}
        if any(isinstance(item, exr.Stored) for item in hdr):      # exr_inflate="device": every OpenEXR file in one batch
            which = [i for i, item in enumerate(hdr) if isinstance(item, (exr.Payload, exr.Stored))]
            batched = dict(zip(which, exr.upload_batch([hdr[i] for i in which], self.device)))
        coded = [i for i, item in enumerate(hdr) if isinstance(item, hdr_io.Scanlines)]       # hdr_rle="device": one batch as well
        decoded = dict(zip(coded, hdr_io.rle_decode_device([hdr[i] for i in coded], self.device)))
        for i, (item, (h, w)) in enumerate(zip(hdr, shapes)):
            out = self.hdr_arena[3 * offsets[i]:3 * (offsets[i] + h * w)].view(h, w, 3)
            if isinstance(item, (exr.Payload, exr.Stored)):        # HALF / FLOAT converted on the device, the file's values
                planes, chunk_offsets = batched[i] if i in batched else exr.upload(item, self.device)
                exr.load_resize(item, planes, chunk_offsets, out, "RGB", clip=False)
            elif i in decoded or (item.dtype == np.uint8 and item.shape[2] == 4):      # RGBE bytes: decoded on the device (a same-size
                tmp = torch.empty_like(out)                                            # "resize" is an exact copy), BGR -> the records' RGB
                K.hdr_load_resize(decoded[i] if i in decoded else torch.from_numpy(item).to(self.device), tmp)
                out.copy_(K.reverse3(tmp))
            else:
                if item.shape[2] != 3:
                    raise ValueError("HdrRealFolder: HDR image %d must be [H, W, 3]" % i)
                out.copy_(torch.from_numpy(item))
        # candidates of every file in the reference's writing order, then ONE statistics launch over all of them
        self.candidates = [(f, h1, w1) for f, (h, w) in enumerate(shapes) for h1, w1 in enumerate_patches(h, w, self.size, self.stride)]
        self._images_dev = torch.from_numpy(self.images).to(self.device)
        if self.candidates:
            cand = np.asarray(self.candidates, dtype=np.int32).reshape(-1, 3)
            count, mean = K.pair_patch_stats(self.ldr_arena, self.hdr_arena, self.images, self._images_dev, cand,
                                             torch.from_numpy(cand).to(self.device), self.size)
            self.extreme_counts, self.means = count.cpu().numpy(), mean.cpu().numpy()
        else:
            self.extreme_counts, self.means = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)
        self.keep = self.extreme_counts <= self.size * self.size // 2                              # convert_to_tf_record.py:56
        self.patches = [c for c, k in zip(self.candidates, self.keep) if k]
        # the gather's tables hold the kept patches only: a sample's patch index is an index into self.patches
        self._patch_table = np.asarray(self.patches, dtype=np.int32).reshape(-1, 3)
        self._patches_dev = torch.from_numpy(self._patch_table).to(self.device)
        self._means_dev = torch.from_numpy(np.ascontiguousarray(self.means[self.keep])).to(self.device)
        torch.cuda.synchronize(self.device)
        self.load_seconds = {"host_decode": host_seconds, "device": time.perf_counter() - t0}
        self.device_bytes = self.ldr_arena.numel() + 4 * self.hdr_arena.numel()
        self._perm_rng = np.random.default_rng([int(seed), 0])                 # the epoch's permutation: the same on every rank
        self.rng = np.random.default_rng([int(seed), 1, self.rank])            # this rank's flips and rotations
        self._queue = []

    def pair(self, file_idx):
        """the resident pair of one file: (uint8 RGB, float32 RGB) views [H, W, 3] of the arenas, on the device"""
        h, w = self.shapes[file_idx]
        o = int(self.images[file_idx, 0])
        return self.ldr_arena[3 * o:3 * (o + h * w)].view(h, w, 3), self.hdr_arena[3 * o:3 * (o + h * w)].view(h, w, 3)

    def host_pair(self, file_idx):
        """the same on the host, as NumPy arrays (write_tfrecords reads them)"""
        l, h = self.pair(file_idx)
        return l.cpu().numpy(), h.cpu().numpy()

    # --- epochs ----------------------------------------------------------------------------------------------------
    def _share(self):
        """this rank's patch indices of the next epoch"""
        return self._perm_rng.permutation(len(self.patches))[self.rank::self.world_size]

    def _augment(self, idx):
        idx = np.asarray(idx, dtype=np.int32).reshape(-1)
        p = np.zeros((idx.size, 3), dtype=np.int32)
        p[:, S_PATCH] = idx
        if self.augment:
            u = self.rng.random((idx.size, 2)).astype(np.float32)                # tfrecord.HdrRealDataset._to_device
            p[:, S_FLIP] = u[:, 0] < 0.5                                         # finetune_real_dataset.py:54-55
            p[:, S_ROT] = (u[:, 1] * 4 + 0.5).astype(np.int32)                   # :58; 4 occurs and is a full turn
        return p

    def draw(self, b=None):
        """the sample table of the next batch of this rank: int32 [b, 3] (patch, flip, rot); epochs follow one another"""
        b = self.batch_size if b is None else int(b)
        if b <= 0 or not self.patches:
            raise ValueError("draw: b must be positive and the folder must hold a kept patch")
        while len(self._queue) < b:
            share = self._share().tolist()
            if not share:                                      # fewer kept patches than ranks: this rank's share can be empty
                raise ValueError("draw: rank %d of %d has no patch (%d kept)" % (self.rank, self.world_size, len(self.patches)))
            self._queue.extend(share)
        idx, self._queue = self._queue[:b], self._queue[b:]
        return self._augment(idx)

    def epoch(self):
        """the sample tables of one epoch of this rank, batch by batch (host)"""
        share = self._share()
        return [self._augment(share[i:i + self.batch_size]) for i in range(0, share.size, self.batch_size)]

    def __len__(self):
        """batches of one epoch of this rank"""
        mine = len(range(self.rank, len(self.patches), self.world_size))
        return -(-mine // self.batch_size)

    def __iter__(self):
        for params in self.epoch():
            yield self.render(params)

    def render(self, params):
        """params int [b, 3] (index into self.patches, flip 0 / 1, rot 0 .. 4), host -> (ref_LDR, ref_HDR), float32
        [b, size, size, 3] on the device.  libshdr checks the table before it launches."""
        if not self.patches:
            raise ValueError("render: the folder holds no kept patch")
        return K.pair_patch_gather(self.ldr_arena, self.hdr_arena, self.images, self._images_dev, self._patch_table, self._patches_dev,
                                   self._means_dev, params, self.size)


def write_tfrecords(folder, out_dir, records_per_file=RECORDS_PER_FILE):
    """The converter, convert_to_tf_record.py without TensorFlow or cv2: the kept patches of `folder`, in order, as GZIP TFRecords
    of tf.train.Example{ref_HDR, ref_LDR} -- the raw bytes of float32 RGB patches, HDR as read, LDR 0 .. 255 -- in files
    train_{stride}_{index:04d}.tfrecords of `records_per_file` records (:42-48).  Returns the written paths.  `folder` is an
    HdrRealFolder, or anything with its `patches`, `size`, `stride` and `host_pair(file)`.

    Not reproduced: at its first patch the reference calls writer.close() on a global that was never assigned, a NameError
    there.  Needs no counterpart: when a patch that the filter drops follows a full file, the reference reopens (and so rewrites
    from empty) file k only at the next kept patch, which is the file's first record anyway."""
    records_per_file = int(records_per_file)
    if records_per_file <= 0:
        raise ValueError("write_tfrecords: records_per_file must be positive")
    os.makedirs(out_dir, exist_ok=True)
    size = folder.size
    cache = {}

    def example(patch):
        f, h1, w1 = patch
        if f not in cache:
            cache.clear()                                      # patches come file by file
            cache[f] = folder.host_pair(f)
        ldr, hdr = cache[f]
        return tfrecord.make_example({
            "ref_HDR": np.ascontiguousarray(hdr[h1:h1 + size, w1:w1 + size], dtype="<f4").tobytes(),
            "ref_LDR": np.ascontiguousarray(ldr[h1:h1 + size, w1:w1 + size], dtype="<f4").tobytes()})

    paths = []
    patches = list(folder.patches)
    for k in range(0, len(patches), records_per_file):
        path = os.path.join(out_dir, "train_%d_%04d.tfrecords" % (folder.stride, k // records_per_file))
        tfrecord.write_records(path, (example(p) for p in patches[k:k + records_per_file]))
        paths.append(path)
    return paths
