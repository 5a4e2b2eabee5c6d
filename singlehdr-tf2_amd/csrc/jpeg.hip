// Baseline-JPEG file decoder on gfx950: the entropy-coded scan of a batch of files -> quantised coefficients -> uint8 RGB,
// bit for bit what libjpeg(-turbo) gives with its defaults (islow IDCT, fancy upsampling).  The host (jpeg.py) parses the
// markers, removes the FF 00 stuffing, cuts the scan at its RSTn markers and builds the Huffman look-up tables; every bit and
// every sample is handled here.
//
// A restart segment (the whole scan of a file without DRI) is one sequential Huffman stream.  It is decoded in parallel with
// the self-synchronising scheme of Weissenberger & Schmidt ("Massively Parallel Huffman Decoding on GPUs", ICPP 2018; its
// JPEG form, 2021): the segment is cut into subsequences of SUB_BITS bits, one thread each.
//
//  * jpeg_sync_kernel    : pass 0: every thread decodes its subsequence from an ASSUMED decoder state (first block of an MCU,
//                          coefficient 0, first bit of the subsequence) and records the state it ends in -- bit position (it
//                          overshoots into the next subsequence: that is where the next code word starts), block in the MCU,
//                          coefficient index -- and how many blocks it completed.  Then, to a fixed point inside the
//                          workgroup: a thread whose left neighbour's end state changed re-decodes from that state.  The first
//                          subsequence of a segment starts from the true state, so after k rounds the first k+1 are final
//                          whatever the data; Huffman codes re-synchronise, and DESIGN.md section 9 has the measured share per round.
//                          The host repeats the launch (pass 1, 2, ...) until no workgroup's last end state changed: the
//                          states cross workgroups through a double-buffered carry array, so a pass reads only what the
//                          previous launch wrote.  Worst case: as many passes as workgroups, a sequential chain, still right.
//  * scan_*_kernel       : inclusive prefix sum (blocks completed per subsequence; later the DC differences).
//  * jpeg_write_kernel   : every thread decodes its subsequence once more from its final start state and writes: AC
//                          coefficients de-zigzagged into the coefficient arena, DC differences in scan order into a flat array.
//  * jpeg_dc_kernel      : DC value = prefix sum of the differences, restarted at every restart interval.
//  * jpeg_idct_kernel    : dequantise, islow IDCT, range-limit: 8 blocks per wavefront -> padded component planes.
//  * jpeg_finish_kernel  : upsample the chroma planes (h2v2 / h2v1 fancy, or replication where libjpeg replicates), YCbCr -> RGB,
//                          crop to W x H.
// No atomics anywhere: the same bytes give the same bits.  Every stream read is clamped to its segment, every coefficient write
// to its image's blocks; an image whose stream is damaged gets an error code and garbage pixels, its neighbours are untouched.
#include "shdr_internal.h"
#include "batch.h"
#include "jpeg_int.h"

namespace {

using namespace shdr::jpegint;

constexpr int WG = 256;
constexpr int SCAN_CHUNK = 1024;                    // elements per scan workgroup (4 per thread)
constexpr int QUANT_BYTES = 4 * 64 * 2;             // per image: four quantisation tables, uint16, natural order
constexpr int SEG_FIELDS = SHDR_JPEG_SEG_FIELDS;

struct Huff {                                       // one table as the host lays it out (jpeg.py device_huffman)
  uint16_t look[512];                               // 9-bit peek -> length << 8 | symbol, 0: the code is longer than 9 bits
  int32_t maxcode[17];                              // largest code of length l (-1: none), l = 1..16
  int32_t valoff[17];                               // index of the first symbol of length l minus its code
  uint8_t val[256];
};
static_assert(sizeof(Huff) == SHDR_JPEG_HUFF_BYTES, "Huffman table layout");
constexpr int TABLE_BYTES = QUANT_BYTES + 4 * (int)sizeof(Huff);
static_assert(TABLE_BYTES == SHDR_JPEG_TABLE_BYTES, "table arena layout");
static_assert(sizeof(shdr_jpeg_image) == 208 && sizeof(shdr_jpeg_batch) == 144, "descriptor layout (jpeg.py mirrors it)");

__constant__ uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the unstuffed stream of one segment: big-endian bit order, read as whole aligned dwords; past the end it reads as 1-bits
struct Bits {
  const uint32_t* d;
  uint32_t ndw, ci;
  uint64_t w;
  __device__ __forceinline__ uint32_t ld(uint32_t i) const { return i < ndw ? __builtin_bswap32(d[i]) : 0xFFFFFFFFu; }
  __device__ __forceinline__ void seek(uint32_t p) {
    ci = p >> 5;
    w = ((uint64_t)ld(ci) << 32) | ld(ci + 1);
  }
  __device__ __forceinline__ uint32_t peek32(uint32_t p) {     // the 32 bits that start at bit p
    const uint32_t i = p >> 5;
    if (i != ci) {
      if (i == ci + 1) { w = (w << 32) | ld(i + 1); ci = i; }
      else seek(p);
    }
    return (uint32_t)(w >> (32 - (p & 31)));
  }
};

__device__ __forceinline__ uint64_t pack_state(uint32_t p, int b, int z) { return ((uint64_t)p << 16) | ((uint64_t)b << 8) | (uint64_t)z; }

struct Layout {                // what the decoder needs of the image, in registers
  int bpm;                     // blocks per MCU
  uint32_t slots;              // 4 bits per block of the MCU: DC table slot | AC table slot << 2
  uint32_t comps;              // 2 bits per block of the MCU: its component
};

__device__ __forceinline__ Layout make_layout(const shdr_jpeg_image* im) {
  Layout L;
  L.bpm = im->blocks_per_mcu;
  L.slots = 0;
  L.comps = 0;
  int b = 0;
  for (int c = 0; c < im->ncomp; ++c)
    for (int k = 0; k < im->comp[c].h * im->comp[c].v && b < 8; ++k, ++b) {
      L.slots |= (uint32_t)((im->comp[c].dc_slot & 3) | ((im->comp[c].ac_slot & 3) << 2)) << (4 * b);
      L.comps |= (uint32_t)c << (2 * b);
    }
  return L;
}

struct Writer {                // the write pass: where block Bi of the image's scan goes
  const shdr_jpeg_image* im;
  int16_t* coef;               // the image's coefficients
  int32_t* dcdiff;             // the image's DC differences, scan order per component
  int Bi, Bend;                // next block (scan order, image-relative) and the end of the segment
  int err;
  long cpos, dpos;
  __device__ __forceinline__ void locate(int b, uint32_t comps) {
    const int c = (comps >> (2 * b)) & 3;
    const int h = im->comp[c].h, hv = h * im->comp[c].v;
    const int m = Bi / im->blocks_per_mcu;
    const int r = c == 0 ? b : 0;
    const int mx = m % im->mcus_x, my = m / im->mcus_x;
    dpos = (long)im->comp[c].blk_off + (long)m * hv + r;
    cpos = (long)im->comp[c].blk_off + (long)(my * im->comp[c].v + r / h) * im->comp[c].bw + mx * h + r % h;
  }
};

// decode from (p, b, z) to the end of the subsequence.  Returns the end state; n = blocks completed.  WRITE: also store.
template <bool WRITE>
__device__ __forceinline__ uint64_t decode_run(const Huff* huff, Bits& bits, const Layout& L, uint32_t p, int b, int z, uint32_t sub_end,
                                               uint32_t seg_bits, int& n, Writer* wr) {
  n = 0;
  if constexpr (WRITE) wr->locate(b, L.comps);
  while (p < sub_end) {
    if constexpr (WRITE) {
      if (wr->Bi >= wr->Bend) break;                            // the segment's blocks are complete: the rest is padding
    }
    const uint32_t slot = (L.slots >> (4 * b)) >> (z == 0 ? 0 : 2) & 3;
    const Huff& H = huff[slot];
    const uint32_t v = bits.peek32(p);
    int len, sym;
    const uint32_t look = H.look[v >> 23];
    if (look) {
      len = look >> 8;
      sym = look & 255;
    } else {
      len = 10;
      int code = (int)(v >> 22);
      while (len <= 16 && code > H.maxcode[len]) {
        ++len;
        code = (int)(v >> (32 - len));
      }
      if (len > 16) {                                            // no such code
        if constexpr (WRITE) { wr->err = SHDR_JPEG_E_CODE; break; }
        len = 16;
        sym = 0;
      } else {
        sym = H.val[(code + H.valoff[len]) & 255];
      }
    }
    int s = z == 0 ? sym : (sym & 15);
    const int r = z == 0 ? 0 : (sym >> 4);
    if (s > 15) {                                                // a DC category baseline JPEG does not have
      if constexpr (WRITE) { wr->err = SHDR_JPEG_E_CODE; break; }
      s = 15;
    }
    int val = 0;
    if (s) {
      const int extra = (int)((v << len) >> (32 - s));          // len + s <= 31
      val = extra < (1 << (s - 1)) ? extra - (1 << s) + 1 : extra;
    }
    p += len + s;
    if constexpr (WRITE) {
      if (p > seg_bits) { wr->err = SHDR_JPEG_E_BITS; break; }  // the code word runs past the end of the segment
    }
    if (z == 0) {
      if constexpr (WRITE) wr->dcdiff[wr->dpos] = val;
      z = 1;
    } else if (s == 0) {
      z = r == 15 ? z + 16 : 64;                                 // ZRL / EOB
    } else {
      z += r;
      if (z > 63) {
        if constexpr (WRITE) { wr->err = SHDR_JPEG_E_OVERRUN; break; }
        z = 64;
      } else {
        if constexpr (WRITE) wr->coef[wr->cpos * 64 + kNatural[z]] = (int16_t)val;
        ++z;
      }
    }
    if (z >= 64) {
      z = 0;
      b = b + 1 == L.bpm ? 0 : b + 1;
      ++n;
      if constexpr (WRITE) {
        ++wr->Bi;
        if (wr->Bi < wr->Bend) wr->locate(b, L.comps);
      }
    }
  }
  return pack_state(p, b, z);
}

struct Sub {                   // one thread's subsequence
  bool valid, first;
  uint32_t p0, end, seg_bits;
  int seg;
  Bits bits;
};

template <int SUB_BITS>
__device__ __forceinline__ Sub load_sub(const uint32_t* data, const int32_t* segs, const int32_t* sub_seg, long g) {
  Sub s;
  s.seg = sub_seg[g];
  s.valid = s.seg >= 0;
  s.first = true;
  s.p0 = s.end = s.seg_bits = 0;
  s.bits.d = data;
  s.bits.ndw = 0;
  if (s.valid) {
    const int32_t* sg = segs + (long)s.seg * SEG_FIELDS;
    const uint32_t k = (uint32_t)(g - sg[SHDR_JPEG_SEG_FIRST_SUB]);
    s.seg_bits = (uint32_t)sg[SHDR_JPEG_SEG_BITS];
    s.p0 = k * SUB_BITS;
    s.end = min(s.p0 + SUB_BITS, s.seg_bits);
    s.first = k == 0;
    s.bits.d = data + sg[SHDR_JPEG_SEG_DWORD];
    s.bits.ndw = (s.seg_bits + 31) >> 5;
  }
  s.bits.seek(s.p0);
  return s;
}

__device__ __forceinline__ void stage_tables(Huff* huff, const uint8_t* tables, const shdr_jpeg_image* im) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tables + im->table_off + QUANT_BYTES);
  uint32_t* dst = reinterpret_cast<uint32_t*>(huff);
  for (int i = threadIdx.x; i < 4 * (int)sizeof(Huff) / 4; i += WG) dst[i] = src[i];
}

// grid = subsequences / 256; every workgroup lies inside one image
template <int SUB_BITS>
__global__ __launch_bounds__(WG) void jpeg_sync_kernel(const uint32_t* __restrict__ data, const uint8_t* __restrict__ tables,
                                                       const shdr_jpeg_image* __restrict__ images, const int32_t* __restrict__ segs,
                                                       const int32_t* __restrict__ sub_seg, uint64_t* __restrict__ state,
                                                       uint64_t* __restrict__ last_in, int32_t* __restrict__ nblk,
                                                       int32_t* __restrict__ settle, uint64_t* __restrict__ carry,
                                                       int32_t* __restrict__ flags, int pass) {
  __shared__ Huff huff[4];
  __shared__ uint64_t st[WG];
  const int t = threadIdx.x, wg = blockIdx.x, nwg = gridDim.x;
  const long g = (long)wg * WG + t;
  const shdr_jpeg_image* im = images + segs[(long)sub_seg[(long)wg * WG] * SEG_FIELDS + SHDR_JPEG_SEG_IMAGE];
  stage_tables(huff, tables, im);
  const Layout L = make_layout(im);
  Sub s = load_sub<SUB_BITS>(data, segs, sub_seg, g);
  const uint64_t assumed = pack_state(s.p0, 0, 0);
  const int par = pass & 1;
  uint64_t carry_in = assumed, mine = assumed;
  int n = 0, when = 0;
  __syncthreads();
  if (pass == 0) {
    uint64_t out = 0;
    if (s.valid) out = decode_run<false>(huff, s.bits, L, s.p0, 0, 0, s.end, s.seg_bits, n, nullptr);
    st[t] = out;
  } else {
    st[t] = state[g];
    mine = last_in[g];
    n = nblk[g];
    when = settle[g];
    if (t == 0 && wg > 0) carry_in = carry[(long)(par ^ 1) * nwg + wg - 1];
  }
  for (int it = 1; it <= WG + 1; ++it) {
    __syncthreads();
    const uint64_t in = t == 0 ? carry_in : st[t - 1];
    const bool need = s.valid && !s.first && in != mine;
    __syncthreads();
    int changed = 0;
    if (need) {
      const uint64_t out = decode_run<false>(huff, s.bits, L, (uint32_t)(in >> 16), (int)(in >> 8) & 255, (int)in & 255, s.end,
                                             s.seg_bits, n, nullptr);
      mine = in;
      if (out != st[t]) {
        st[t] = out;
        changed = 1;
        when = pass * (WG + 2) + it;
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  state[g] = st[t];
  last_in[g] = mine;
  nblk[g] = n;
  settle[g] = when;
  if (t == WG - 1) {
    carry[(long)par * nwg + wg] = st[t];
    if (pass > 0 && st[t] != carry[(long)(par ^ 1) * nwg + wg]) flags[pass] = 1;     // (every writer stores the same value)
  }
}

// ---------------------------------------------------------------- inclusive scan: out[i] + partial[i / SCAN_CHUNK]
// (the sums are unsigned: the DC sums of a batch wrap around by design, only differences of two of them are used)
__global__ __launch_bounds__(WG) void scan_local_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out,
                                                        int32_t* __restrict__ partial, long n) {
  __shared__ uint32_t wsum[4];
  const long i0 = (long)blockIdx.x * SCAN_CHUNK + threadIdx.x * 4;
  uint32_t v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = i0 + k < n ? (uint32_t)in[i0 + k] : 0u;
  v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
  const uint32_t base = shdr::block_scan<WG>(v[3], wsum);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < n) out[i0 + k] = (int32_t)(v[k] + base);
  if (threadIdx.x == WG - 1) partial[blockIdx.x] = (int32_t)(base + v[3]);
}

// one workgroup: partial[] -> its exclusive prefix sum, in place
__global__ __launch_bounds__(WG) void scan_partials_kernel(int32_t* __restrict__ partial, long n) {
  shdr::scan_array<WG, 1>(
      n, [&](int64_t i) { return (uint32_t)partial[i]; }, [&](int64_t i, uint32_t before) { partial[i] = (int32_t)before; });
}

__device__ __forceinline__ uint32_t scanned(const int32_t* __restrict__ out, const int32_t* __restrict__ partial, long i) {
  return (uint32_t)out[i] + (uint32_t)partial[i / SCAN_CHUNK];
}

// ---------------------------------------------------------------- the write pass
template <int SUB_BITS>
__global__ __launch_bounds__(WG) void jpeg_write_kernel(const uint32_t* __restrict__ data, const uint8_t* __restrict__ tables,
                                                        const shdr_jpeg_image* __restrict__ images, const int32_t* __restrict__ segs,
                                                        const int32_t* __restrict__ sub_seg, const uint64_t* __restrict__ state,
                                                        const int32_t* __restrict__ nblk, const int32_t* __restrict__ incl,
                                                        const int32_t* __restrict__ partial, int16_t* __restrict__ coef,
                                                        int32_t* __restrict__ dcdiff, int32_t* __restrict__ wg_err) {
  __shared__ Huff huff[4];
  __shared__ int errs[WG];
  const int t = threadIdx.x, wg = blockIdx.x;
  const long g = (long)wg * WG + t;
  const shdr_jpeg_image* im = images + segs[(long)sub_seg[(long)wg * WG] * SEG_FIELDS + SHDR_JPEG_SEG_IMAGE];
  stage_tables(huff, tables, im);
  const Layout L = make_layout(im);
  Sub s = load_sub<SUB_BITS>(data, segs, sub_seg, g);
  __syncthreads();
  int err = 0;
  if (s.valid) {
    const int32_t* sg = segs + (long)s.seg * SEG_FIELDS;
    const long f = sg[SHDR_JPEG_SEG_FIRST_SUB];
    Writer wr;
    wr.im = im;
    wr.coef = coef + im->blk_off * 64;
    wr.dcdiff = dcdiff + im->blk_off;
    wr.err = 0;
    wr.Bend = sg[SHDR_JPEG_SEG_FIRST_BLOCK] + sg[SHDR_JPEG_SEG_BLOCKS];
    // blocks completed by the subsequences of this segment before this one
    // (fewer than 2^20 slots of at most 2048 bits, a block takes two bits or more: the sum stays below 2^31 whatever the bytes say)
    const long before = (long)(scanned(incl, partial, g) - (uint32_t)nblk[g]) - (long)(scanned(incl, partial, f) - (uint32_t)nblk[f]);
    const long Bi = sg[SHDR_JPEG_SEG_FIRST_BLOCK] + before;
    if (before < 0 || Bi >= wr.Bend) {
      // nothing left for this subsequence: the segment's blocks ended before it (padding, or a damaged stream reported by
      // the subsequence that ran out)
    } else {
      wr.Bi = (int)Bi;
      uint32_t p = s.p0;
      int b = 0, z = 0, n;
      if (!s.first) {
        const uint64_t in = state[g - 1];
        p = (uint32_t)(in >> 16); b = (int)(in >> 8) & 255; z = (int)in & 255;
      }
      if (b >= L.bpm || z > 63 || b != (int)(Bi % L.bpm)) {
        err = SHDR_JPEG_E_CODE;                                   // a start state the true chain cannot produce
      } else {
        decode_run<true>(huff, s.bits, L, p, b, z, s.end, s.seg_bits, n, &wr);
        err = wr.err;
        // the last subsequence of the segment must complete the segment's blocks
        if (!err && s.end == s.seg_bits && wr.Bi < wr.Bend) err = SHDR_JPEG_E_BITS;
      }
    }
    if (s.seg_bits == 0 && s.first && sg[SHDR_JPEG_SEG_BLOCKS] > 0) err = SHDR_JPEG_E_BITS;
  }
  errs[t] = err;
  __syncthreads();
  if (t == 0) {
    int e = 0;
    for (int k = 0; k < WG && !e; ++k) e = errs[k];
    wg_err[wg] = e;
  }
}

// one thread per image: the first error of its workgroups
__global__ void jpeg_errors_kernel(const shdr_jpeg_image* __restrict__ images, const int32_t* __restrict__ wg_err,
                                   int32_t* __restrict__ errors, int n_images) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_images) return;
  int e = 0;
  for (int k = 0; k < images[i].n_wg && !e; ++k) e = wg_err[images[i].first_wg + k];
  errors[i] = e;
}

__device__ __forceinline__ int find_image(const shdr_jpeg_image* __restrict__ images, int n_images, long blk) {
  int lo = 0, hi = n_images - 1;                     // the last image whose blk_off <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (images[mid].blk_off <= blk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one thread per block, in the order of dcdiff (image, component, scan order): DC = sum of the differences since the restart
__global__ __launch_bounds__(WG) void jpeg_dc_kernel(const shdr_jpeg_image* __restrict__ images, int n_images,
                                                     const int32_t* __restrict__ incl, const int32_t* __restrict__ partial,
                                                     int16_t* __restrict__ coef, long n_blocks) {
  const long k = (long)blockIdx.x * WG + threadIdx.x;
  if (k >= n_blocks) return;
  const shdr_jpeg_image* im = images + find_image(images, n_images, k);
  const int rel = (int)(k - im->blk_off);
  int c = 0;
  while (c + 1 < im->ncomp && rel >= im->comp[c + 1].blk_off) ++c;
  const int j = rel - im->comp[c].blk_off;
  const int h = im->comp[c].h, hv = h * im->comp[c].v;
  if (j >= im->mcus_x * im->mcus_y * hv) return;
  const int per = im->restart_interval > 0 ? im->restart_interval * hv : 0x7FFFFFFF;
  const long k0 = k - j + (long)(j / per) * per;                     // first block of this restart interval
  const int dc = (int)(scanned(incl, partial, k) - (k0 > 0 ? scanned(incl, partial, k0 - 1) : 0u));
  const int m = j / hv, r = j % hv;
  const int mx = m % im->mcus_x, my = m / im->mcus_x;
  const long pos = (long)im->comp[c].blk_off + (long)(my * im->comp[c].v + r / h) * im->comp[c].bw + mx * h + r % h;
  coef[(im->blk_off + pos) * 64] = (int16_t)dc;
}

// 64 threads = 8 blocks of the coefficient arena (raster order inside a component) -> the component's padded plane
__global__ __launch_bounds__(64) void jpeg_idct_kernel(const shdr_jpeg_image* __restrict__ images, int n_images,
                                                       const uint8_t* __restrict__ tables, const int16_t* __restrict__ coef,
                                                       uint8_t* __restrict__ planes, long n_blocks) {
  __shared__ int ws[8][64];
  __shared__ long dst[8];            // byte offset of the block's first sample in `planes`, -1: no such block
  __shared__ long quant[8];          // byte offset of its quantisation table in `tables`
  __shared__ int pitch[8];
  const int t = threadIdx.x;
  const long k0 = (long)blockIdx.x * 8;
  if (t < 8) {
    const long k = k0 + t;
    dst[t] = -1;
    if (k < n_blocks) {
      const shdr_jpeg_image* im = images + find_image(images, n_images, k);
      const int rel = (int)(k - im->blk_off);
      int c = 0;
      while (c + 1 < im->ncomp && rel >= im->comp[c + 1].blk_off) ++c;
      const int j = rel - im->comp[c].blk_off, bw = im->comp[c].bw;
      if (j < bw * im->comp[c].bh) {
        pitch[t] = bw * 8;
        dst[t] = im->plane_off + im->comp[c].plane_off + (long)(j / bw) * 8 * pitch[t] + (j % bw) * 8;
        quant[t] = im->table_off + im->comp[c].tq * 128;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i)
    ws[i][t] = dst[i] >= 0 ? (int)coef[(k0 + i) * 64 + t] * (int)reinterpret_cast<const uint16_t*>(tables + quant[i])[t] : 0;
  __syncthreads();
  idct_1d(&ws[t >> 3][t & 7], 8, true);
  __syncthreads();
  idct_1d(&ws[t >> 3][(t & 7) * 8], 1, false);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (dst[i] >= 0) planes[dst[i] + (long)(t >> 3) * pitch[i] + (t & 7)] = clamp_u8(ws[i][t] + 128);
}

// grid = (pixels / 256 capped, images)
__global__ __launch_bounds__(WG) void jpeg_finish_kernel(const shdr_jpeg_image* __restrict__ images, const uint8_t* __restrict__ planes,
                                                         uint8_t* __restrict__ out) {
  const shdr_jpeg_image* im = images + blockIdx.y;
  const int W = im->width, H = im->height;
  const long npix = (long)W * H;
  const uint8_t* yp = planes + im->plane_off + im->comp[0].plane_off;
  const int ypitch = im->comp[0].bw * 8;
  uint8_t* o = out + im->out_off;
  if (im->ncomp == 1) {
    for (long p = (long)blockIdx.x * WG + threadIdx.x; p < npix; p += (long)gridDim.x * WG) {
      const int y = (int)(p / W), x = (int)(p - (long)y * W);
      const uint8_t v = yp[(long)y * ypitch + x];
      o[p * 3] = v; o[p * 3 + 1] = v; o[p * 3 + 2] = v;
    }
    return;
  }
  const uint8_t* cb = planes + im->plane_off + im->comp[1].plane_off;
  const uint8_t* cr = planes + im->plane_off + im->comp[2].plane_off;
  const int cpitch = im->comp[1].bw * 8, cw = im->comp[1].cw, ch = im->comp[1].ch;
  const int hs = im->comp[0].h, vs = im->comp[0].v;
  const bool fancy = cw > 2;                                    // jdsample.c: narrower planes are replicated
  for (long p = (long)blockIdx.x * WG + threadIdx.x; p < npix; p += (long)gridDim.x * WG) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const int yy = yp[(long)y * ypitch + x];
    int u, v;
    if (hs == 1) {                                              // 4:4:4
      u = cb[(long)y * cpitch + x];
      v = cr[(long)y * cpitch + x];
    } else if (!fancy) {
      const long q = (long)(vs == 2 ? y >> 1 : y) * cpitch + (x >> 1);
      u = cb[q];
      v = cr[q];
    } else if (vs == 1) {                                       // 4:2:2
      u = fancy_up_h2v1(cb + (long)y * cpitch, cw, x);
      v = fancy_up_h2v1(cr + (long)y * cpitch, cw, x);
    } else {                                                    // 4:2:0
      u = fancy_up_h2v2(cb, cpitch, ch, cw, y, x);
      v = fancy_up_h2v2(cr, cpitch, ch, cw, y, x);
    }
    int r, g, b;
    ycc_to_rgb(yy, u - 128, v - 128, r, g, b);
    o[p * 3] = (uint8_t)r; o[p * 3 + 1] = (uint8_t)g; o[p * 3 + 2] = (uint8_t)b;
  }
}

inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

struct Workspace {             // byte offsets into the caller's workspace
  int64_t state, last_in, carry, nblk, settle, incl, partial, flags, wg_err, dcdiff, dcincl, dcpartial, planes, end, zero_end;
};

Workspace layout(int64_t n_sub, int64_t n_blocks, int64_t plane_bytes) {
  const int64_t nwg = n_sub / WG;
  Workspace w;
  int64_t o = 0;
  // zero-filled before every decode: the pass flags and the DC differences of blocks a damaged stream never reaches
  w.flags = o; o = up256(o + 4 * (nwg + 2));
  w.dcdiff = o; o = up256(o + 4 * n_blocks);
  w.zero_end = o;
  w.state = o; o = up256(o + 8 * n_sub);
  w.last_in = o; o = up256(o + 8 * n_sub);
  w.carry = o; o = up256(o + 16 * nwg);
  w.nblk = o; o = up256(o + 4 * n_sub);
  w.settle = o; o = up256(o + 4 * n_sub);
  w.incl = o; o = up256(o + 4 * n_sub);
  w.partial = o; o = up256(o + 4 * ((n_sub + SCAN_CHUNK - 1) / SCAN_CHUNK));
  w.wg_err = o; o = up256(o + 4 * nwg);
  w.dcincl = o; o = up256(o + 4 * n_blocks);
  w.dcpartial = o; o = up256(o + 4 * ((n_blocks + SCAN_CHUNK - 1) / SCAN_CHUNK));
  w.planes = o; o = up256(o + plane_bytes);
  w.end = o;
  return w;
}

using Stages = shdr::StageTimer<SHDR_JPEG_STAGES>;                // shdr_jpeg_batch.stage_ms: a mark() behind every stage

void scan(const int32_t* in, int32_t* out, int32_t* partial, int64_t n, hipStream_t st) {
  const int64_t chunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
  hipLaunchKernelGGL(scan_local_kernel, dim3((unsigned)chunks), dim3(WG), 0, st, in, out, partial, (long)n);
  hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(WG), 0, st, partial, (long)chunks);
}

// the tables as the kernels trust them: every index they form from these lies inside the caller's buffers
int validate(const shdr_jpeg_batch* b) {
  SHDR_REQUIRE(b && b->data && b->tables && b->images && b->images_dev && b->segs && b->segs_dev && b->sub_seg && b->sub_seg_dev,
               SHDR_E_NULL, "jpeg: null pointer");
  SHDR_REQUIRE(b->n_images > 0 && b->n_images <= 65535 && b->n_segs > 0 && b->n_sub > 0 && b->n_sub % WG == 0 &&
               b->n_sub < (int64_t)1 << 20 && b->n_blocks > 0 && b->n_blocks < (int64_t)1 << 25 && b->data_bytes % 4 == 0 &&
               b->data_bytes < (int64_t)1 << 33 && b->plane_bytes >= 0,
               SHDR_E_SHAPE, "jpeg: bad batch sizes (%d images, %d segments, %lld subsequences, %lld blocks, %lld bytes)", b->n_images,
               b->n_segs, (long long)b->n_sub, (long long)b->n_blocks, (long long)b->data_bytes);
  SHDR_REQUIRE(b->subseq_bits == 256 || b->subseq_bits == 512 || b->subseq_bits == 1024 || b->subseq_bits == 2048, SHDR_E_SHAPE,
               "jpeg: subsequence length %d (256, 512, 1024 and 2048 bits are compiled)", b->subseq_bits);
  for (int i = 0; i < b->n_images; ++i) {
    const shdr_jpeg_image& im = b->images[i];
    bool ok = im.width > 0 && im.height > 0 && (im.ncomp == 1 || im.ncomp == 3) && im.mcus_x > 0 && im.mcus_y > 0 &&
              im.restart_interval >= 0 && im.blk_off >= 0 && im.plane_off >= 0 && im.out_off >= 0 && im.table_off >= 0 &&
              im.table_off % 4 == 0 && im.table_off + TABLE_BYTES <= b->table_bytes && im.first_wg >= 0 && im.n_wg > 0 &&
              (int64_t)(im.first_wg + im.n_wg) * WG <= b->n_sub && (int64_t)im.mcus_x * im.mcus_y < (1 << 24) &&
              im.out_off + (int64_t)im.width * im.height * 3 <= b->out_bytes;
    SHDR_REQUIRE(ok, SHDR_E_SHAPE, "jpeg: image %d: bad descriptor", i);
    SHDR_REQUIRE(i == 0 || im.blk_off > b->images[i - 1].blk_off, SHDR_E_SHAPE, "jpeg: image %d: block offsets must increase", i);
    SHDR_REQUIRE(im.first_wg == (i == 0 ? 0 : b->images[i - 1].first_wg + b->images[i - 1].n_wg), SHDR_E_SHAPE,
                 "jpeg: image %d: its workgroups must follow those of image %d without a gap or an overlap", i, i - 1);
    int bpm = 0;
    int64_t blocks = 0, planes = 0;
    for (int c = 0; c < im.ncomp; ++c) {
      const auto& k = im.comp[c];
      ok = ((k.h == 1 && k.v == 1) || (c == 0 && im.ncomp == 3 && k.h == 2 && (k.v == 1 || k.v == 2))) && k.tq >= 0 && k.tq < 4 &&
           k.dc_slot >= 0 && k.dc_slot < 4 && k.ac_slot >= 0 && k.ac_slot < 4 && k.bw == im.mcus_x * k.h &&
           k.bh == im.mcus_y * k.v && k.blk_off == blocks && k.plane_off == planes && k.cw > 0 && k.cw <= k.bw * 8 && k.ch > 0 &&
           k.ch <= k.bh * 8;
      SHDR_REQUIRE(ok, SHDR_E_SHAPE, "jpeg: image %d component %d: bad descriptor", i, c);
      bpm += k.h * k.v;
      blocks += (int64_t)k.bw * k.bh;
      planes += (int64_t)k.bw * k.bh * 64;
    }
    ok = bpm == im.blocks_per_mcu && im.blk_off + blocks <= b->n_blocks && im.plane_off + planes <= b->plane_bytes &&
         im.width <= im.comp[0].bw * 8 && im.height <= im.comp[0].bh * 8 &&
         (im.ncomp == 1 || (im.comp[1].cw * im.comp[0].h >= im.width && im.comp[1].ch * im.comp[0].v >= im.height));
    SHDR_REQUIRE(ok, SHDR_E_SHAPE, "jpeg: image %d: the components do not cover the image or overrun the arenas", i);
  }
  SHDR_REQUIRE((int64_t)(b->images[b->n_images - 1].first_wg + b->images[b->n_images - 1].n_wg) * WG == b->n_sub, SHDR_E_SHAPE,
               "jpeg: the images' workgroups do not cover the %lld subsequence slots", (long long)b->n_sub);
  for (int s = 0; s < b->n_segs; ++s) {
    const int32_t* sg = b->segs + (int64_t)s * SEG_FIELDS;
    const int img = sg[SHDR_JPEG_SEG_IMAGE];
    SHDR_REQUIRE(img >= 0 && img < b->n_images, SHDR_E_SHAPE, "jpeg: segment %d: image %d", s, img);
    const shdr_jpeg_image& im = b->images[img];
    const int64_t bits = (uint32_t)sg[SHDR_JPEG_SEG_BITS], subs = bits ? (bits + b->subseq_bits - 1) / b->subseq_bits : 1;
    const int64_t first = sg[SHDR_JPEG_SEG_FIRST_SUB];
    const bool ok = sg[SHDR_JPEG_SEG_DWORD] >= 0 && bits < ((int64_t)1 << 31) &&
                    ((int64_t)sg[SHDR_JPEG_SEG_DWORD] + (bits + 31) / 32) * 4 <= b->data_bytes &&
                    first >= (int64_t)im.first_wg * WG && first + subs <= (int64_t)(im.first_wg + im.n_wg) * WG &&
                    sg[SHDR_JPEG_SEG_FIRST_BLOCK] >= 0 && sg[SHDR_JPEG_SEG_BLOCKS] >= 0 &&
                    (int64_t)sg[SHDR_JPEG_SEG_FIRST_BLOCK] + sg[SHDR_JPEG_SEG_BLOCKS] <=
                        (int64_t)im.mcus_x * im.mcus_y * im.blocks_per_mcu;
    SHDR_REQUIRE(ok, SHDR_E_SHAPE, "jpeg: segment %d: bad descriptor", s);
  }
  for (int64_t g = 0; g < b->n_sub; ++g) {
    const int s = b->sub_seg[g];
    if (s < 0) {
      SHDR_REQUIRE(g % WG != 0, SHDR_E_SHAPE, "jpeg: subsequence %lld: a workgroup must start with a subsequence", (long long)g);
      continue;
    }
    SHDR_REQUIRE(s < b->n_segs, SHDR_E_SHAPE, "jpeg: subsequence %lld: segment %d", (long long)g, s);
    const int32_t* sg = b->segs + (int64_t)s * SEG_FIELDS;
    const int64_t k = g - sg[SHDR_JPEG_SEG_FIRST_SUB], bits = (uint32_t)sg[SHDR_JPEG_SEG_BITS];
    const shdr_jpeg_image& im = b->images[sg[SHDR_JPEG_SEG_IMAGE]];
    SHDR_REQUIRE(k >= 0 && (k == 0 || k * b->subseq_bits < bits) && g / WG >= im.first_wg && g / WG < im.first_wg + im.n_wg &&
                 (k == 0 || b->sub_seg[g - 1] == s),
                 SHDR_E_SHAPE, "jpeg: subsequence %lld does not lie in segment %d", (long long)g, s);
  }
  return SHDR_OK;
}

template <int SUB_BITS>
int entropy(const shdr_jpeg_batch* b, int16_t* coef, int32_t* errors, char* ws, const Workspace& w, hipStream_t st, Stages& stages) {
  const int nwg = (int)(b->n_sub / WG);
  const uint32_t* data = reinterpret_cast<const uint32_t*>(b->data);
  auto* state = reinterpret_cast<uint64_t*>(ws + w.state);
  auto* last_in = reinterpret_cast<uint64_t*>(ws + w.last_in);
  auto* carry = reinterpret_cast<uint64_t*>(ws + w.carry);
  auto* nblk = reinterpret_cast<int32_t*>(ws + w.nblk);
  auto* settle = reinterpret_cast<int32_t*>(ws + w.settle);
  auto* incl = reinterpret_cast<int32_t*>(ws + w.incl);
  auto* partial = reinterpret_cast<int32_t*>(ws + w.partial);
  auto* flags = reinterpret_cast<int32_t*>(ws + w.flags);
  auto* wg_err = reinterpret_cast<int32_t*>(ws + w.wg_err);
  auto* dcdiff = reinterpret_cast<int32_t*>(ws + w.dcdiff);
  auto* dcincl = reinterpret_cast<int32_t*>(ws + w.dcincl);
  auto* dcpartial = reinterpret_cast<int32_t*>(ws + w.dcpartial);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)w.zero_end, st);
  if (e == hipSuccess) e = hipMemsetAsync(coef, 0, (size_t)b->n_blocks * 128, st);
  if (e != hipSuccess) return shdr::fail(SHDR_E_LAUNCH, "jpeg: memset: %s", hipGetErrorString(e));
  stages.mark();                                                   // SHDR_JPEG_STAGE_CLEAR
  // pass 0 and 1 always run; pass k > 1 only while pass k - 1 changed a workgroup's last end state (at most nwg + 1 passes:
  // each pass makes at least one more workgroup final)
  int passes = 0;
  for (int pass = 0; pass <= nwg + 1; ++pass) {
    hipLaunchKernelGGL(jpeg_sync_kernel<SUB_BITS>, dim3(nwg), dim3(WG), 0, st, data, b->tables, b->images_dev, b->segs_dev, b->sub_seg_dev,
                       state, last_in, nblk, settle, carry, flags, pass);
    ++passes;
    if (pass == 0) continue;
    if (nwg == 1) break;                                           // one workgroup: pass 1 only confirms pass 0
    int32_t flag = 0;
    e = hipMemcpyAsync(&flag, flags + pass, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return shdr::fail(SHDR_E_LAUNCH, "jpeg: synchronisation pass %d: %s", pass, hipGetErrorString(e));
    if (!flag) break;
  }
  if (b->passes) *b->passes = passes;
  stages.mark();                                                   // SHDR_JPEG_STAGE_SYNC
  scan(nblk, incl, partial, b->n_sub, st);
  hipLaunchKernelGGL(jpeg_write_kernel<SUB_BITS>, dim3(nwg), dim3(WG), 0, st, data, b->tables, b->images_dev, b->segs_dev, b->sub_seg_dev,
                     state, nblk, incl, partial, coef, dcdiff, wg_err);
  hipLaunchKernelGGL(jpeg_errors_kernel, dim3((b->n_images + 63) / 64), dim3(64), 0, st, b->images_dev, wg_err, errors, b->n_images);
  stages.mark();                                                   // SHDR_JPEG_STAGE_WRITE
  scan(dcdiff, dcincl, dcpartial, b->n_blocks, st);
  hipLaunchKernelGGL(jpeg_dc_kernel, dim3((unsigned)((b->n_blocks + WG - 1) / WG)), dim3(WG), 0, st, b->images_dev, b->n_images, dcincl,
                     dcpartial, coef, (long)b->n_blocks);
  stages.mark();                                                   // SHDR_JPEG_STAGE_DC
  return shdr::check_launch("jpeg_entropy_decode");
}

int entropy_dispatch(const shdr_jpeg_batch* b, int16_t* coef, int32_t* errors, void* workspace, hipStream_t st, Stages& stages) {
  const Workspace w = layout(b->n_sub, b->n_blocks, b->plane_bytes);
  char* ws = static_cast<char*>(workspace);
  switch (b->subseq_bits) {
    case 256: return entropy<256>(b, coef, errors, ws, w, st, stages);
    case 512: return entropy<512>(b, coef, errors, ws, w, st, stages);
    case 1024: return entropy<1024>(b, coef, errors, ws, w, st, stages);
    default: return entropy<2048>(b, coef, errors, ws, w, st, stages);
  }
}

}  // namespace

extern "C" int64_t shdr_jpeg_workspace_bytes(int64_t n_sub, int64_t n_blocks, int64_t plane_bytes) {
  if (n_sub <= 0 || n_sub % WG != 0 || n_blocks <= 0 || plane_bytes < 0) {
    shdr::fail(SHDR_E_SHAPE, "jpeg_workspace_bytes: need n_sub > 0 (a multiple of %d), n_blocks > 0, plane_bytes >= 0", WG);
    return -1;
  }
  return layout(n_sub, n_blocks, plane_bytes).end;
}

extern "C" int shdr_jpeg_entropy_decode(const shdr_jpeg_batch* batch, int16_t* coef, int32_t* errors, void* workspace, void* stream) {
  if (int rc = validate(batch)) return rc;
  SHDR_REQUIRE(coef && errors && workspace, SHDR_E_NULL, "jpeg_entropy_decode: null pointer");
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "jpeg_entropy_decode: the workspace must be 16-byte aligned");
  Stages stages(batch->stage_ms, shdr::stream_of(stream));
  return entropy_dispatch(batch, coef, errors, workspace, shdr::stream_of(stream), stages);
}

extern "C" int shdr_jpeg_decode_u8(const shdr_jpeg_batch* batch, int16_t* coef, uint8_t* out, int32_t* errors, void* workspace,
                                   void* stream) {
  if (int rc = validate(batch)) return rc;
  SHDR_REQUIRE(coef && out && errors && workspace, SHDR_E_NULL, "jpeg_decode_u8: null pointer");
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "jpeg_decode_u8: the workspace must be 16-byte aligned");
  hipStream_t st = shdr::stream_of(stream);
  Stages stages(batch->stage_ms, st);
  if (int rc = entropy_dispatch(batch, coef, errors, workspace, st, stages)) return rc;
  const Workspace w = layout(batch->n_sub, batch->n_blocks, batch->plane_bytes);
  uint8_t* planes = static_cast<uint8_t*>(workspace) + w.planes;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((batch->n_blocks + 7) / 8)), dim3(64), 0, st, batch->images_dev, batch->n_images,
                     batch->tables, coef, planes, (long)batch->n_blocks);
  stages.mark();                                                   // SHDR_JPEG_STAGE_IDCT
  int64_t maxpix = 0;
  for (int i = 0; i < batch->n_images; ++i) {
    const int64_t p = (int64_t)batch->images[i].width * batch->images[i].height;
    if (p > maxpix) maxpix = p;
  }
  hipLaunchKernelGGL(jpeg_finish_kernel, dim3(shdr::stream_grid(maxpix), batch->n_images), dim3(WG), 0, st, batch->images_dev, planes, out);
  stages.mark();                                                   // SHDR_JPEG_STAGE_FINISH
  return shdr::check_launch("jpeg_decode_u8");
}

// debugging / measurement: the round (pass * 258 + iteration, 0 = the speculative decode was already right) in which each
// subsequence's end state last changed, copied from the workspace of the last decode to a host array of n_sub int32
extern "C" int shdr_jpeg_sync_rounds(const void* workspace, int64_t n_sub, int64_t n_blocks, int64_t plane_bytes, int32_t* rounds,
                                     void* stream) {
  SHDR_REQUIRE(workspace && rounds, SHDR_E_NULL, "jpeg_sync_rounds: null pointer");
  SHDR_REQUIRE(n_sub > 0 && n_sub % WG == 0 && n_blocks > 0 && plane_bytes >= 0, SHDR_E_SHAPE, "jpeg_sync_rounds: bad sizes");
  const Workspace w = layout(n_sub, n_blocks, plane_bytes);
  hipError_t e = hipMemcpyAsync(rounds, static_cast<const char*>(workspace) + w.settle, (size_t)n_sub * 4, hipMemcpyDeviceToHost, shdr::stream_of(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(shdr::stream_of(stream));
  if (e != hipSuccess) return shdr::fail(SHDR_E_LAUNCH, "jpeg_sync_rounds: %s", hipGetErrorString(e));
  return SHDR_OK;
}
