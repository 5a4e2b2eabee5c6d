"""dataset.py of the reference: the HDR training set of joint_training.py:202 and train.py:255.

    from dataset import get_train_dataset, RandDatasetReader          # package directory on sys.path, as in the reference
    reader = RandDatasetReader(get_train_dataset(hdr_dir), 32)
    hdr, crf, invcrf, t = reader.read_batch_data()                     # device tensors [b,256,256,3], [b,1024], [b,1024], [b]

Each file is read once when the dataset is built.  Radiance files: the RLE scanlines are decoded on the host (libshdr, a bounded
thread pool; with hdr_rle="device" on the device, all files in one hdr_io.rle_decode_device), the RGBE bytes go to the device and one kernel decodes, reverses the channels to cv2's BGR and resizes the short
side to 512 into a resident arena.  OpenEXR files (exr.py): the host inflates or run-length decodes the chunks in the same
pool, the device undoes OpenEXR's byte predictor and one kernel converts HALF / FLOAT, clips at 0 (:185), orders the channels
BGR and resizes into the same arena.  A second kernel computes the mean of every 512 x 512 crop.  A batch is then one launch of the
patch sampler (csrc/dataset.hip): crop, normalise, resize to S x S, 256 crop, rot90 and the two flips of
PatchHDRDataset.__getitem__ (dataset.py:212-252), for every sample at once.  The CRF / exposure tables (:19-54) are host
numpy, built once.

cv2 is not a dependency of this project, so its behaviour is restated, not run: cv2.imread('.hdr') is Ward's RGBE decode without
the +0.5 (hdr_io.rgbe_decode), and both `cv2.resize(img, size, cv2.INTER_AREA)` calls (:190, :225) pass the flag as the
positional `dst` argument, so the interpolation in effect is the default INTER_LINEAR -- OpenCV's resize.cpp bilinear rule
(half-pixel centres, edge taps clamped) as written out at the top of csrc/dataset.hip.

Deliberate differences from the reference:
  * Nothing is read at import.  get_*_dataset(hdr_prefix, posfix_list=None, crf_path=None) take the file list; without one
    they use i_dataset_{train,test}.pkl next to this module when present (the reference's lists), else the sorted *.hdr files
    under hdr_prefix.  dorfCurves.txt is looked up as `crf_path`, next to this module, then in the current directory (the
    rule of linearization_net.load_invemor_table); a missing file raises FileNotFoundError.  No DoRF file is shipped.
  * Random draws come from np.random.default_rng keyed by (seed, rank).  The reference's streams cannot be reproduced (24
    forked workers share one np.random.seed(5) state, and its reader permutes the whole 2N x n_crf x n_t index space per
    epoch); here an epoch is a permutation of the 2N patches, and the CRF and exposure are drawn uniformly.  The
    distributions are the reference's.
  * RandDatasetReader(dataset, batch_size, seed=0, rank=0).read_batch_data() returns device tensors, not lists of numpy
    arrays, and starts no worker processes.  It is draw() followed by PatchHDRDataset.render() and the CRF / t gathers.
  * Radiance files (FORMAT=32-bit_rle_rgbe, -Y h +X w) and OpenEXR files are read, chosen by their magic bytes.  Of OpenEXR,
    single-part scanline files with NO_COMPRESSION, RLE, ZIPS or ZIP compression and HALF / FLOAT R, G, B channels (exr.py);
    PIZ files too where exr_piz="host" or "device" asks for them (the default "refuse" raises ValueError; that reader is unpinned:
    no OpenEXR-written PIZ file has been read); PXR24, B44(A), DWAA / DWAB, tiled, deep, multi-part and luminance / chroma files
    raise ValueError.  Alpha and other
    extra channels are ignored: cv2.imread(path, IMREAD_UNCHANGED) would return 4 channels, which the reference's network
    cannot take.  The file list without a .pkl is the sorted *.hdr and *.exr files.
"""
import concurrent.futures
import glob
import os
import pickle
import time
from abc import ABC, abstractmethod

import numpy as np
import torch

try:
    from . import _ops as K
    from . import exr
    from . import hdr_io
except ImportError:
    import _ops as K
    import exr
    import hdr_io

CURR_PATH_PREFIX = os.path.dirname(os.path.abspath(__file__))
DORF_FILE = "dorfCurves.txt"
PATCH = 256                    # the training crop (dataset.py:236)
WINDOW = 512                   # the short side after loading and the crop side (:188, :216-219)
MAX_LOAD_THREADS = 16

# columns of the parameter table of draw() / render(); the first seven are the kernel's (include/shdr.h)
P_IDX, P_S, P_Y0, P_X0, P_K, P_FLIP0, P_FLIP1, P_CRF, P_T = range(9)
N_PARAMS = 9


# --- crf_list, invcrf_list, t_list (dataset.py:19-54) ---------------------------------------------------------------
def _find_dorf(crf_path=None):
    for cand in (crf_path, os.path.join(CURR_PATH_PREFIX, DORF_FILE), DORF_FILE):
        if cand and os.path.isfile(cand):
            return cand
    raise FileNotFoundError("%s not found (looked at %s, next to %s and in %s); pass crf_path=" % (
        DORF_FILE, crf_path, __file__, os.getcwd()))


def _get_crf_list(crf_path=None):
    """(test_crf_list, train_crf_list): the brightness rows (line idx + 5 of every 6), shuffled by RandomState(730), last 10 test"""
    with open(_find_dorf(crf_path), "r") as f:
        lines = [line.strip() for line in f.readlines()]
    crf_list = [lines[idx + 5] for idx in range(0, len(lines), 6)]
    crf_list = np.float32([ele.split() for ele in crf_list])
    np.random.RandomState(730).shuffle(crf_list)
    return crf_list[-10:], crf_list[:-10]


def _inverse_rf(_rf):
    """rf[0] = 0, rf[-1] = 1, then scipy's interp1d(rf, linspace(0, 1, s))(linspace(0, 1, s)) restated: stable sort of the
    abscissae, searchsorted(left) clipped to [1, s-1], slope * (x - x_lo) + y_lo with the differences of rf in its own dtype"""
    rf = _rf.copy()
    s, = rf.shape
    rf[0] = 0.0
    rf[-1] = 1.0
    order = np.argsort(rf, kind="mergesort")
    x, y = rf[order], np.linspace(0.0, 1.0, num=s)[order]
    xn = np.linspace(0.0, 1.0, num=s)
    hi = np.clip(np.searchsorted(x, xn), 1, s - 1)
    lo = hi - 1
    slope = (y[hi] - y[lo]) / (x[hi] - x[lo])
    return slope * (xn - x[lo]) + y[lo]


def _get_invcrf_list(crf_list):
    return np.array([_inverse_rf(crf) for crf in crf_list])


def get_t_list(n):
    return 2 ** np.linspace(-3, 3, n, dtype="float32")


# --- Dataset, MultiDimDataset, MemDataset (dataset.py:58-155) -------------------------------------------------------
class Dataset(ABC):

    @abstractmethod
    def __getitem__(self, idx):
        pass

    @abstractmethod
    def __len__(self):
        pass

    def __iter__(self):
        return DatasetIter(self)


class DatasetIter:

    def __init__(self, dataset):
        self._i = 0
        self._dataset = dataset

    def __iter__(self):
        return self

    def __next__(self):
        if self._i >= len(self._dataset):
            raise StopIteration()
        result = self._dataset[self._i]
        self._i += 1
        return result


class CatDataset(Dataset):

    def __init__(self, dataset_list):
        self.dataset_list = dataset_list
        self._len = len(dataset_list[0])
        for dataset in dataset_list:
            assert self._len == len(dataset)

    def __getitem__(self, idx):
        data_list = []
        for dataset in self.dataset_list:
            data = dataset[idx]
            data_list.extend(data if type(data) is list else [data])
        return data_list

    def __len__(self):
        return self._len


class MergeDataset(Dataset):
    """index = patch fastest, then CRF, then t (dataset.py:124-136)"""

    def __init__(self, dataset_list):
        self.dataset_list = dataset_list
        self._len = 1
        for dataset in dataset_list:
            self._len *= len(dataset)

    def __getitem__(self, all_idx):
        data_list = []
        for dataset in self.dataset_list:
            all_idx, curr_idx = all_idx // len(dataset), all_idx % len(dataset)
            data = dataset[curr_idx]
            data_list.extend(data if type(data) is list else [data])
        assert all_idx == 0
        return data_list

    def __len__(self):
        return self._len


class MemDataset(Dataset):

    def __init__(self, dataset):
        self._arr = [ele for ele in dataset]

    def __getitem__(self, idx):
        return self._arr[idx]

    def __len__(self):
        return len(self._arr)


# --- HDRDataset, PatchHDRDataset (dataset.py:159-268) --------------------------------------------------------------
def _load_pkl(name):
    path = os.path.join(CURR_PATH_PREFIX, name + ".pkl")
    if not os.path.isfile(path):
        return None
    with open(path, "rb") as f:
        return pickle.load(f)


def _source_shape(item):
    """(h, w) of an item of HDRDataset"""
    if isinstance(item, (exr.Payload, exr.Stored)):
        return item.header.height, item.header.width
    return item.shape[:2]                               # RGBE pixels, or hdr_io.Scanlines


def resized_shape(h, w):
    """HDRDataset._hdr_read_resize (:188-191): short side to 512 with Python's round()"""
    ratio = max(WINDOW / h, WINDOW / w)
    return round(h * ratio), round(w * ratio)


def draw_patch_params(idx, rng, is_training):
    """the random draws of PatchHDRDataset.__getitem__ (:224-250) for patch indices idx: int32 [b, 7] (P_IDX ... P_FLIP1);
    without training, S = 512 and no augmentation"""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    b = idx.size
    p = np.zeros((b, 7), dtype=np.int32)
    p[:, P_IDX] = idx
    if not is_training:
        p[:, P_S] = WINDOW
        return p
    S = np.round(WINDOW * rng.uniform(0.5, 2.0, b)).astype(np.int32)          # :224-225
    span = np.maximum(S - PATCH, 1)                                           # randint(0, S - 256): upper bound exclusive
    x0 = rng.integers(0, span)                                                # :233 (x before y)
    y0 = rng.integers(0, span)
    p[:, P_S] = S
    p[:, P_X0] = np.where(S == PATCH, 0, x0)                                  # S == 256: returned uncropped (:230-231)
    p[:, P_Y0] = np.where(S == PATCH, 0, y0)
    p[:, P_K] = rng.integers(0, 4, b)                                         # np.rot90(hdr, randint(4))  (:240)
    p[:, P_FLIP0] = rng.integers(0, 2, b)                                     # :243-245
    p[:, P_FLIP1] = rng.integers(0, 2, b)                                     # :247-249
    return p


class ParamSampler:
    """The draws of RandDatasetReader, host only: an epoch is a permutation of the n_patches patch indices; the CRF and
    exposure indices are uniform.  np.random.default_rng((seed, rank)): every data-parallel rank has its own stream."""

    def __init__(self, n_patches, n_crf, n_t, is_training, seed=0, rank=0):
        self.n_patches, self.n_crf, self.n_t, self.is_training = int(n_patches), int(n_crf), int(n_t), is_training
        self.rng = np.random.default_rng([int(seed), int(rank)])
        self._perm, self._pos = np.zeros(0, dtype=np.int64), 0

    def _next_patches(self, b):
        out = []
        while len(out) < b:
            if self._pos >= self._perm.size:
                self._perm, self._pos = self.rng.permutation(self.n_patches), 0
            take = min(b - len(out), self._perm.size - self._pos)
            out.extend(self._perm[self._pos:self._pos + take].tolist())
            self._pos += take
        return out

    def draw(self, b):
        """int32 [b, N_PARAMS] (columns P_IDX ... P_T)"""
        p = np.zeros((b, N_PARAMS), dtype=np.int32)
        p[:, :7] = draw_patch_params(self._next_patches(b), self.rng, self.is_training)
        p[:, P_CRF] = self.rng.integers(0, self.n_crf, b)
        p[:, P_T] = self.rng.integers(0, self.n_t, b)
        return p


class HDRDataset(Dataset):
    """the file list; items are the RGBE bytes of a Radiance file or the exr.Payload of an OpenEXR one (the pixels are
    converted on the device, see PatchHDRDataset)"""

    def __init__(self, hdr_prefix, hdr_posfix_list, is_training, exr_inflate="host", exr_piz="refuse", hdr_rle="host"):
        """exr_inflate "device": ZIP / ZIPS OpenEXR files come back as exr.Stored (checked, not inflated; exr.upload_batch's input).
        exr_piz: PIZ files are refused ("refuse"), decoded on the host ("host") or come back as exr.Stored too ("device").
        hdr_rle "device": Radiance files come back as hdr_io.Scanlines (header checked, scanlines left coded; hdr_io.rle_decode_device's
        input)"""
        self._hdr_prefix = hdr_prefix
        self._hdr_posfix_list = list(hdr_posfix_list)
        self.is_training = is_training
        self.exr_inflate = exr.check_inflate_option("HDRDataset", exr_inflate)
        self.exr_piz = exr.check_piz_option("HDRDataset", exr_piz)
        self.hdr_rle = hdr_io.check_decoder_option("HDRDataset", hdr_rle)

    def path(self, idx):
        return os.path.join(self._hdr_prefix, self._hdr_posfix_list[idx])

    def __getitem__(self, idx):
        path = self.path(idx)
        if not exr.is_exr(path):
            return hdr_io.read_scanlines(path) if self.hdr_rle == "device" else hdr_io.read_rgbe(path)
        return exr.read_item(path, self.exr_inflate, self.exr_piz)

    def __len__(self):
        return len(self._hdr_posfix_list)


class PatchHDRDataset(Dataset):
    """2 patches per file (:212-252): the first and last 512 rows (portrait) or columns (otherwise) of the resized image,
    normalised to mean 0.5; training adds a random resize, 256 crop, rot90 and flips.  Every file is resident on the device."""

    def __init__(self, hdr_prefix, hdr_posfix_list, is_training, load_to_mem=True, device=None, seed=0, exr_inflate="host",
                 exr_piz="refuse", hdr_rle="host"):
        """load_to_mem is the reference's argument; the images are always resident (on the device).  exr_inflate: who inflates the
        ZIP / ZIPS chunks of OpenEXR files -- "host" (zlib, in the loading threads) or "device" (all files' chunks in one
        exr.upload_batch; the time moves from load_seconds["host_decode"] to load_seconds["device"]); the arena is the same.
        exr_piz: PIZ-compressed OpenEXR files are refused ("refuse", the default), decoded in the loading threads by libshdr's host
        routine ("host") or on the device, in that same batch ("device", K.piz_decode); the arena is the same either way.
        hdr_rle: who decodes the scanlines of Radiance files -- "host" (shdr_rgbe_rle_decode, in the loading threads, then one upload
        of 4 B / pixel per file) or "device" (the coded bytes of all files in one upload and one hdr_io.rle_decode_device; the time
        moves from load_seconds["host_decode"] to load_seconds["device"]); the arena is the same"""
        self._hdr_dataset = HDRDataset(hdr_prefix, hdr_posfix_list, is_training, exr_inflate, exr_piz, hdr_rle)
        self._is_training = is_training
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.rng = np.random.default_rng(seed)          # draws of __getitem__ (the reader has its own)
        self.load_seconds = {}
        self._load()

    @property
    def is_training(self):
        return self._is_training

    @property
    def patch_size(self):
        return PATCH if self._is_training else WINDOW

    def _load(self):
        n = len(self._hdr_dataset)
        if n == 0:
            raise ValueError("PatchHDRDataset: empty file list")
        t0 = time.perf_counter()
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(MAX_LOAD_THREADS, n)) as pool:     # ctypes, zlib drop the GIL
            items = list(pool.map(self._hdr_dataset.__getitem__, range(n)))
        t1 = time.perf_counter()
        shapes = [resized_shape(*_source_shape(r)) for r in items]
        sizes = [h * w * 3 for h, w in shapes]
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.arena = torch.empty(int(sum(sizes)), device=self.device, dtype=torch.float32)
        batched = {}
        if self._hdr_dataset.exr_inflate == "device" or any(isinstance(r, exr.Stored) for r in items):     # every OpenEXR file in one batch
            which = [i for i, r in enumerate(items) if isinstance(r, (exr.Payload, exr.Stored))]
            batched = dict(zip(which, exr.upload_batch([items[i] for i in which], self.device)))
        coded = [i for i, r in enumerate(items) if isinstance(r, hdr_io.Scanlines)]           # hdr_rle="device": every Radiance file in one batch
        decoded = dict(zip(coded, hdr_io.rle_decode_device([items[i] for i in coded], self.device)))
        for i, (r, (h, w)) in enumerate(zip(items, shapes)):
            out = self.arena[offsets[i]:offsets[i] + sizes[i]].view(h, w, 3)
            if isinstance(r, (exr.Payload, exr.Stored)):
                planes, chunk_offsets = batched[i] if i in batched else exr.upload(r, self.device)
                exr.load_resize(r, planes, chunk_offsets, out, "BGR", clip=True)
            else:
                K.hdr_load_resize(decoded[i] if i in decoded else torch.from_numpy(r).to(self.device), out)
        self.shapes = shapes
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self.dims = torch.tensor(shapes, dtype=torch.int32).to(self.device)
        self.means = K.hdr_window_means(self.arena, self.offsets, self.dims)
        torch.cuda.synchronize(self.device)
        self.load_seconds = {"host_decode": t1 - t0, "device": time.perf_counter() - t1}
        self._offsets_host = offsets

    def image(self, file_idx):
        """the resident image of one file: float32 BGR [H, W, 3] on the device"""
        h, w = self.shapes[file_idx]
        o = int(self._offsets_host[file_idx])
        return self.arena[o:o + h * w * 3].view(h, w, 3)

    def __len__(self):
        return 2 * len(self._hdr_dataset)

    def draw(self, idx, rng):
        return draw_patch_params(idx, rng, self._is_training)

    def check_params(self, params):
        p = np.asarray(params)
        if p.ndim != 2 or p.shape[1] < 7:
            raise ValueError("render: params must be [b, >= 7]")
        P = self.patch_size
        idx, S, y0, x0, k, f0, f1 = (p[:, c] for c in range(7))
        bad = ((idx < 0) | (idx >= len(self)) | (S < P) | (y0 < 0) | (x0 < 0) | (y0 + P > S) | (x0 + P > S) | (k < 0) | (k > 3)
               | ((f0 != 0) & (f0 != 1)) | ((f1 != 0) & (f1 != 1)))
        if not self._is_training:
            bad |= (S != WINDOW) | (k != 0) | (f0 != 0) | (f1 != 0)
        if bad.any():
            raise ValueError("render: invalid parameter row %s" % p[int(np.argmax(bad))].tolist())

    def render(self, params):
        """params [b, >= 7] (numpy, or an int32 device tensor already checked) -> float32 [b, P, P, 3] on the device, P = 256
        when training, 512 otherwise"""
        if not isinstance(params, torch.Tensor):
            params = np.ascontiguousarray(params, dtype=np.int32)
            self.check_params(params)
            host = torch.from_numpy(params).pin_memory()
            params = host.to(self.device, non_blocking=True)
        return K.hdr_patch_sample(self.arena, self.offsets, self.dims, self.means, params, self.patch_size)

    def __getitem__(self, idx):
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        return self.render(self.draw([idx], self.rng))[0]


# --- get_train_dataset, get_vali_dataset, get_i_test_dataset (dataset.py:271-313) ----------------------------------
def _posfix_list(hdr_prefix, posfix_list, pkl_name):
    if posfix_list is None:
        posfix_list = _load_pkl(pkl_name)
    if posfix_list is None:
        posfix_list = sorted(os.path.relpath(p, hdr_prefix) for ext in ("*.hdr", "*.exr")
                             for p in glob.glob(os.path.join(hdr_prefix, ext)))
        if not posfix_list:
            raise FileNotFoundError("no %s.pkl next to %s and no *.hdr or *.exr under %s" % (pkl_name, __file__, hdr_prefix))
    return list(posfix_list)


def crf_tables(split, crf_path=None):
    """(crf, invcrf, t) of get_train_dataset / get_vali_dataset / get_i_test_dataset (:271-313): split 'train', 'vali' or 'test'"""
    test_crf_list, train_crf_list = _get_crf_list(crf_path)
    if split == "train":
        return train_crf_list, _get_invcrf_list(train_crf_list), get_t_list(600)
    if split == "test":
        return test_crf_list, _get_invcrf_list(test_crf_list), get_t_list(7)
    if split == "vali":
        def _rand_rf_list(rf_list):
            rf_list = rf_list.copy()
            np.random.RandomState(730).shuffle(rf_list)
            return np.array(rf_list[:10])
        return _rand_rf_list(test_crf_list), _rand_rf_list(_get_invcrf_list(test_crf_list)), get_t_list(5)
    raise ValueError("split must be 'train', 'vali' or 'test'")


def _merge(patches, tables):
    crf, invcrf, t = tables
    return MergeDataset([patches, CatDataset([crf, invcrf]), t])


def get_train_dataset(hdr_prefix, posfix_list=None, crf_path=None, device=None, exr_inflate="host", exr_piz="refuse", hdr_rle="host"):
    tables = crf_tables("train", crf_path)                     # first: a missing DoRF file fails before any file is loaded
    return _merge(PatchHDRDataset(hdr_prefix, _posfix_list(hdr_prefix, posfix_list, "i_dataset_train"), True, device=device,
                                  exr_inflate=exr_inflate, exr_piz=exr_piz, hdr_rle=hdr_rle), tables)


def get_vali_dataset(hdr_prefix, posfix_list=None, crf_path=None, device=None, exr_inflate="host", exr_piz="refuse", hdr_rle="host"):
    tables = crf_tables("vali", crf_path)
    posfix_list = _posfix_list(hdr_prefix, posfix_list, "i_dataset_test")
    np.random.RandomState(730).shuffle(posfix_list)
    return _merge(PatchHDRDataset(hdr_prefix, posfix_list[:10], False, device=device, exr_inflate=exr_inflate, exr_piz=exr_piz, hdr_rle=hdr_rle), tables)


def get_i_test_dataset(hdr_prefix, posfix_list=None, crf_path=None, device=None, exr_inflate="host", exr_piz="refuse", hdr_rle="host"):
    tables = crf_tables("test", crf_path)
    return _merge(PatchHDRDataset(hdr_prefix, _posfix_list(hdr_prefix, posfix_list, "i_dataset_test"), False, device=device,
                                  exr_inflate=exr_inflate, exr_piz=exr_piz, hdr_rle=hdr_rle), tables)


# --- RandDatasetReader (dataset.py:318-363) -------------------------------------------------------------------------
class RandDatasetReader:
    """Batches of a get_*_dataset() result on the device: [hdr [b,P,P,3], crf [b,1024], invcrf [b,1024], t [b]] (P = 256 for
    training, 512 otherwise), ready for camera.CameraPipeline(hdr, crf, t) and pipeline.JointTrainStep(ds, invcrf).
    read_batch_data() = render(draw()); the draws are a ParamSampler's."""

    def __init__(self, dataset, batch_size, seed=0, rank=0):
        patches, rf, t_list = dataset.dataset_list
        crf, invcrf = rf.dataset_list
        self.patches, self._batch_size = patches, int(batch_size)
        dev = patches.device
        self.crf = torch.from_numpy(np.ascontiguousarray(crf, dtype=np.float32)).to(dev)
        self.invcrf = torch.from_numpy(np.ascontiguousarray(invcrf, dtype=np.float32)).to(dev)
        self.t = torch.from_numpy(np.ascontiguousarray(t_list, dtype=np.float32)).to(dev)
        self.sampler = ParamSampler(len(patches), len(crf), len(t_list), patches.is_training, seed, rank)

    def draw(self, b=None):
        """the parameters of the next batch: int32 [b, N_PARAMS] (columns P_IDX ... P_T)"""
        return self.sampler.draw(self._batch_size if b is None else int(b))

    def render(self, params):
        """[hdr, crf, invcrf, t] on the device for a parameter table of draw(); one pinned copy, one sampler launch"""
        params = np.ascontiguousarray(params, dtype=np.int32)
        self.patches.check_params(params)
        if params.shape[1] < N_PARAMS or ((params[:, P_CRF] < 0) | (params[:, P_CRF] >= self.crf.shape[0]) | (params[:, P_T] < 0)
                                          | (params[:, P_T] >= self.t.shape[0])).any():
            raise ValueError("render: CRF or exposure index missing or out of range")
        dparams = torch.from_numpy(params).pin_memory().to(self.patches.device, non_blocking=True)
        hdr = self.patches.render(dparams)
        ci, ti = dparams[:, P_CRF].contiguous(), dparams[:, P_T].contiguous()
        return [hdr, self.crf.index_select(0, ci), self.invcrf.index_select(0, ci), self.t.index_select(0, ti)]

    def read_batch_data(self):
        return self.render(self.draw())
