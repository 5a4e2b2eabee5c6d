// Baseline-JPEG writer on the device: the files of shdr_jpeg_encode_host (csrc/api.cpp), byte for byte, for a BATCH of 8-bit RGB images
// of different sizes, layouts, qualities and restart intervals.  Every rule -- block grid, edges, quantiser, zig-zag, the Annex-K
// tables, the bits of a block, segments, padding, stuffing -- is csrc/jpeg_enc.h, shared with the host twin.
//
// Passes (stream-ordered, no global atomics, no host wait, no allocation; the same input gives the same bytes):
//   0  enc_setup_kernel      first MCU / block / segment / pixel of every image, status words cleared            (1 thread, N steps)
//   1  enc_transform_kernel  one wave per MCU: colour conversion, box filter, islow FDCT, quantiser -> int16 [blocks][64], zig-zag
//                            order, MCU scan order, dummy blocks included (as jpeg_mcu_kernel of camera.hip, for the three layouts
//                            and the edge rules)
//   2  enc_bits_kernel       one lane per block: its coded bits given its predecessor's DC; an out-of-range coefficient sets the
//                            image's status word
//   3  enc_scan_kernel       exclusive scan of the bits over all blocks; enc_segments_kernel: one lane per restart segment, its
//                            unstuffed byte count and its first word in the arena.  Segment S (counted over the batch) starts at word
//                            (bits before it >> 5) + S: word-aligned, in order, never overlapping, and no scan over segments is needed
//   4  enc_write_kernel      the unstuffed bit stream: a workgroup takes 120 consecutive blocks, each lane codes one block and ORs its
//                            codes into an LDS image of the tile's words (integer OR is order-independent); the tile stores whole
//                            words, each word of the arena exactly once: the word a tile shares with the one before it belongs to the
//                            later tile, whose first 8 lanes code the earlier tile's last 8 blocks again and keep what falls into that
//                            word (a block has at least 4 bits, so no more than 8 reach into its 31 bits)
//   5  enc_ff_count_kernel   FF bytes per 1 KiB of the arena, and their exclusive scan
//   6  enc_sizes_kernel      one lane per segment: its stuffed size (+ the header in front of an image's first, + the RSTn / EOI
//                            marker behind it); their exclusive scan gives every segment's final offset and the images' offsets
//   7  enc_final_kernel      one lane per arena word: its bytes at their final offsets with a 00 after every FF, and the marker behind
//                            a segment's last byte, put together in an LDS window and stored as whole words (bytes only where a word
//                            is shared with another tile or with a header); enc_header_kernel: the host-composed headers and offsets[]
// Compiled with -ffp-contract=off (the float input is quantised as jpeg_mcu_kernel does).
#include <string.h>

#include "shdr_internal.h"
#include "batch.h"
#include "jpeg_enc.h"

namespace {

using namespace jpegenc;
using namespace shdr::jpegint;

constexpr int kTileBlocks = 120;                                  // blocks a workgroup of enc_write_kernel owns
constexpr int kCarryBlocks = 8;                                   // + the lanes for the blocks before them: ceil(31 bits / 4 bits per block)
constexpr int kTileWords = (kTileBlocks + kCarryBlocks) * (kBlockWords + 2) + 8;       // its bits / 32 + a gap per segment start
constexpr int kFfTile = 1024;                                     // arena bytes per FF count: 256 lanes x one word
constexpr int kStageWords = 672;                                  // LDS window of enc_final_kernel: a tile's 1024 bytes, a 00 behind each,
                                                                  // a marker per word (segments start on words), and the alignment

__device__ const CodeTables d_codes = kCodes;

struct EncWorkspace {                          // carved out of the caller's workspace, every part 16-byte aligned
  int64_t *mcu0, *blk0, *seg0, *pix0;          // [N + 1] first MCU, block, segment and pixel of image n among all of the batch
  int16_t* coef;                               // [B][64]
  int32_t* bits;                               // [B]
  int64_t* bitpos;                             // [B + 1]
  int64_t* segword;                            // [S + 1] first arena word of every segment; [S]: the words used
  int32_t* segbytes;                           // [S] unstuffed bytes
  int64_t* segff;                              // [S] FF bytes of the arena before the segment
  int64_t* segsize;                            // [S] bytes of the output that belong to the segment
  int64_t* segout;                             // [S + 1] where they start
  uint32_t* arena;                             // [arena_words] the unstuffed scan, bytes in stream order
  int32_t* ffcnt;                              // [T] FF bytes per kFfTile
  int64_t* ffscan;                             // [T + 1]
  int64_t arena_words, ff_tiles, bytes;
};
inline EncWorkspace carve(void* ws, int64_t n, int64_t blocks, int64_t segs) {
  EncWorkspace w;
  shdr::Carver cut(ws);
  w.mcu0 = cut.take<int64_t>(n + 1);
  w.blk0 = cut.take<int64_t>(n + 1);
  w.seg0 = cut.take<int64_t>(n + 1);
  w.pix0 = cut.take<int64_t>(n + 1);
  w.coef = cut.take<int16_t>(64 * blocks);
  w.bits = cut.take<int32_t>(blocks);
  w.bitpos = cut.take<int64_t>(blocks + 1);
  w.segword = cut.take<int64_t>(segs + 1);
  w.segbytes = cut.take<int32_t>(segs);
  w.segff = cut.take<int64_t>(segs);
  w.segsize = cut.take<int64_t>(segs);
  w.segout = cut.take<int64_t>(segs + 1);
  w.arena_words = blocks * kBlockWords + segs + 2;
  w.ff_tiles = (w.arena_words * 4 + kFfTile - 1) / kFfTile;
  w.arena = cut.take<uint32_t>(w.ff_tiles * (kFfTile / 4));      // whole tiles: the count reads them whole
  w.ffcnt = cut.take<int32_t>(w.ff_tiles);
  w.ffscan = cut.take<int64_t>(w.ff_tiles + 1);
  w.bytes = cut.bytes();
  return w;
}

__global__ void enc_setup_kernel(const Image* __restrict__ images, int n, int64_t* __restrict__ mcu0, int64_t* __restrict__ blk0,
                                 int64_t* __restrict__ seg0, int64_t* __restrict__ pix0, int32_t* __restrict__ status) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t m = 0, b = 0, s = 0, p = 0;
  for (int i = 0; i < n; ++i) {
    const Image im = images[i];
    const Geometry g = geometry(im);
    mcu0[i] = m; blk0[i] = b; seg0[i] = s; pix0[i] = p;
    status[i] = kOk;
    m += g.mcus; b += g.blocks; s += g.segments; p += (int64_t)im.height * im.width;
  }
  mcu0[n] = m; blk0[n] = b; seg0[n] = s; pix0[n] = p;
}

__device__ __forceinline__ int sample_u8(const uint8_t* p) { return *p; }
__device__ __forceinline__ int sample_u8(const float* p) { return (int)fminf(fmaxf(rintf(*p * 255.0f), 0.0f), 255.0f); }

// grid = the MCUs of the batch; block = 64 threads (one wavefront) = one MCU
template <typename T>
__global__ __launch_bounds__(64) void enc_transform_kernel(const T* __restrict__ pixels, const Image* __restrict__ images, int n,
                                                           const int64_t* __restrict__ mcu0, const int64_t* __restrict__ blk0,
                                                           const int64_t* __restrict__ pix0, int16_t* __restrict__ coef) {
  __shared__ int blk[6][64];      // the MCU's blocks in scan order, [row][col] of each
  __shared__ int cfull[2][256];   // full-resolution Cb, Cr of the MCU, rows of 8 h samples
  __shared__ __align__(16) int16_t zq[6][64];   // quantised, zig-zag order
  const int lane = threadIdx.x;
  const int64_t m = blockIdx.x;
  const int i = (int)shdr::last_le(mcu0, n, m);
  const Image im = images[i];
  const Geometry g = geometry(im);
  const int ml = (int)(m - mcu0[i]);
  const int my = ml / g.mcus_x, mx = ml - my * g.mcus_x;
  const int mw = 8 * g.h, mh = 8 * g.v;
  const T* img = pixels + pix0[i] * 3;
  for (int p = lane; p < mw * mh; p += 64) {
    const int py = p / mw, px = p - py * mw;
    const T* s = img + ((int64_t)imin(my * mh + py, im.height - 1) * im.width + imin(mx * mw + px, im.width - 1)) * 3;
    int y, cb, cr;
    rgb_to_ycc(sample_u8(s), sample_u8(s + 1), sample_u8(s + 2), y, cb, cr);
    blk[(py >> 3) * g.h + (px >> 3)][(py & 7) * 8 + (px & 7)] = y - 128;
    cfull[0][p] = cb;
    cfull[1][p] = cr;
  }
  __syncthreads();
  {  // lane = chroma sample (cy, cx).  The rows of cfull are already clamped to H - 1, the columns to W - 1 (chroma_src_row / _col)
    const int cy = lane >> 3, cx = lane & 7;
    const int col = mx * 8 + cx;
    const int py = g.v * imin(my * 8 + cy, g.crows - 1) - my * mh;            // the MCU row of the (upper) full-resolution row
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int* c = cfull[k] + py * mw + g.h * cx;
      const int val = g.hv == 4 ? box_h2v2(c[0], c[1], c[mw], c[mw + 1], col) : g.hv == 2 ? box_h2v1(c[0], c[1], col) : c[0];
      blk[g.hv + k][lane] = val - 128;
    }
  }
  __syncthreads();
  if (lane < g.nbm * 8) fdct_1d(&blk[lane >> 3][(lane & 7) * 8], 1, true);
  __syncthreads();
  if (lane < g.nbm * 8) fdct_1d(&blk[lane >> 3][lane & 7], 8, false);
  __syncthreads();
  const int zp = zigzag_position(lane);
  for (int b = 0; b < g.nbm; ++b) {
    const bool dummy = b < g.hv && y_block_dummy(g, my, mx, b);
    zq[b][zp] = dummy ? (int16_t)0 : (int16_t)quantise(blk[b][lane], quant_value(lane, b >= g.hv, im.quality));
  }
  __syncthreads();
  if (lane == 0)
    for (int b = 1; b < g.hv; ++b)
      if (y_block_dummy(g, my, mx, b)) zq[b][0] = zq[b - 1][0];
  __syncthreads();
  uint32_t* dst = reinterpret_cast<uint32_t*>(coef) + (blk0[i] + (int64_t)ml * g.nbm) * 32;
  for (int w = lane; w < g.nbm * 32; w += 64) dst[w] = reinterpret_cast<const uint32_t*>(&zq[0][0])[w];
}

// a block's 64 coefficients in registers: 8 loads of 16 bytes
struct BlockRegs {
  uint32_t w[32];
  __device__ __forceinline__ void load(const int16_t* __restrict__ p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 v = q[k];
      w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
  }
  __device__ __forceinline__ int operator()(int k) const { return (int)(int16_t)(w[k >> 1] >> (16 * (k & 1))); }
};

// what the lanes need to know about block b of the batch
struct BlockInfo {
  int image;
  int64_t local;                               // its number in the image
  int64_t seg;                                 // its segment, counted over the batch
  int64_t seg_first;                           // that segment's first block, counted over the batch
  int pred;                                    // the DC it is predicted from
  bool chroma, last_of_segment;
};
__device__ __forceinline__ BlockInfo block_info(int64_t b, const Image* __restrict__ images, int n, const int64_t* __restrict__ blk0,
                                                const int64_t* __restrict__ seg0, const int16_t* __restrict__ coef) {
  BlockInfo r;
  r.image = (int)shdr::last_le(blk0, n, b);
  const Image im = images[r.image];
  const Geometry g = geometry(im);
  r.local = b - blk0[r.image];
  const int64_t s = segment_of_block(g, im.restart, r.local);
  r.seg = seg0[r.image] + s;
  r.seg_first = blk0[r.image] + segment_first_block(g, im.restart, s);
  const int64_t pb = pred_block(g, im.restart, r.local);
  r.pred = pb < 0 ? 0 : (int)coef[(blk0[r.image] + pb) * 64];
  r.chroma = block_is_chroma(g, r.local);
  r.last_of_segment = r.local + 1 == segment_first_block(g, im.restart, s + 1);
  return r;
}

__global__ __launch_bounds__(256) void enc_bits_kernel(const int16_t* __restrict__ coef, const Image* __restrict__ images, int n,
                                                       const int64_t* __restrict__ blk0, const int64_t* __restrict__ seg0,
                                                       int32_t* __restrict__ bits, int32_t* __restrict__ status) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= blk0[n]) return;
  const BlockInfo info = block_info(b, images, n, blk0, seg0, coef);
  BlockRegs zz;
  zz.load(coef + b * 64);
  int total = 0;
  const bool ok = code_block(d_codes, zz, info.pred, info.chroma, [&](uint32_t, int len) { total += len; });
  bits[b] = ok ? total : 0;
  if (!ok) status[info.image] = kOutOfRange;                        // every lane that stores here stores the same word
}

// out[i] = sum of in[0 .. i), out[n] = the total.  One block.
template <typename T>
__global__ __launch_bounds__(1024) void enc_scan_kernel(const T* __restrict__ in, int64_t n, int64_t* __restrict__ out) {
  const int64_t all = shdr::scan_array<1024, 4>(
      n, [&](int64_t i) { return (int64_t)in[i]; }, [&](int64_t i, int64_t before) { out[i] = before; });
  if (threadIdx.x == 0) out[n] = all;
}

// one lane per segment of the batch (+ one for the end of the arena)
__global__ __launch_bounds__(256) void enc_segments_kernel(const Image* __restrict__ images, int n, const int64_t* __restrict__ blk0,
                                                           const int64_t* __restrict__ seg0, const int64_t* __restrict__ bitpos,
                                                           int64_t* __restrict__ segword, int32_t* __restrict__ segbytes) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nseg = seg0[n];
  if (s > nseg) return;
  if (s == nseg) {
    segword[s] = (bitpos[blk0[n]] >> 5) + nseg;
    return;
  }
  const int i = (int)shdr::last_le(seg0, n, s);
  const Image im = images[i];
  const Geometry g = geometry(im);
  const int64_t fb = blk0[i] + segment_first_block(g, im.restart, s - seg0[i]);
  const int64_t lb = blk0[i] + segment_first_block(g, im.restart, s - seg0[i] + 1);
  segword[s] = (bitpos[fb] >> 5) + s;
  segbytes[s] = (int32_t)((bitpos[lb] - bitpos[fb] + 7) >> 3);
}

// the arena bit at which block b starts
__device__ __forceinline__ int64_t block_start_bit(int64_t b, const BlockInfo& info, const int64_t* __restrict__ bitpos,
                                                   const int64_t* __restrict__ segword) {
  return segword[info.seg] * 32 + (bitpos[b] - bitpos[info.seg_first]);
}

// grid = ceil(B / kTileBlocks); block = 128 threads: lane t >= 8 codes block tile * 120 + t - 8, lanes 0 .. 7 the 8 blocks before the tile
__global__ __launch_bounds__(128) void enc_write_kernel(const int16_t* __restrict__ coef, const Image* __restrict__ images, int n,
                                                        const int64_t* __restrict__ blk0, const int64_t* __restrict__ seg0,
                                                        const int64_t* __restrict__ bitpos, const int64_t* __restrict__ segword,
                                                        const int32_t* __restrict__ status,
                                                        uint32_t* __restrict__ arena, int64_t arena_words) {
  __shared__ uint32_t tile[kTileWords];
  const int64_t nblk = blk0[n], nseg = seg0[n];
  const int64_t first = (int64_t)blockIdx.x * kTileBlocks;
  const int64_t next = first + kTileBlocks;
  // the words of this tile: from the word in which its first block starts to the word in which the next tile's first block starts
  const BlockInfo finfo = block_info(first, images, n, blk0, seg0, coef);
  const int64_t w_first = block_start_bit(first, finfo, bitpos, segword) >> 5;
  int64_t w_end = segword[nseg];
  if (next < nblk) w_end = block_start_bit(next, block_info(next, images, n, blk0, seg0, coef), bitpos, segword) >> 5;
  int64_t nwords = w_end - w_first;
  if (nwords > kTileWords) nwords = kTileWords;                    // (never: kTileWords is the bound of 128 blocks and their gaps)
  for (int w = threadIdx.x; w < nwords; w += 128) tile[w] = 0;
  __syncthreads();
  const int64_t b = first + (int64_t)threadIdx.x - kCarryBlocks;
  if (b >= 0 && b < next && b < nblk) {
    const BlockInfo info = block_info(b, images, n, blk0, seg0, coef);
    // lanes 0 .. 7: only a block of the first block's segment reaches into this tile's first word
    if ((threadIdx.x >= kCarryBlocks || info.seg == finfo.seg) && status[info.image] == kOk) {
      BlockRegs zz;
      zz.load(coef + b * 64);
      const int64_t rel = block_start_bit(b, info, bitpos, segword) - w_first * 32;      // < 0 for lanes 0 .. 7
      int wi = (int)(rel >> 5), o = (int)(rel & 31);               // the word being filled and the bits of it that are taken
      uint64_t acc = 0;                                            // that word in the high half, its successor below
      auto flush = [&]() {
        if (wi >= 0 && wi < nwords) atomicOr(&tile[wi], (uint32_t)(acc >> 32));
        acc <<= 32;
        ++wi;
        o -= 32;
      };
      auto put = [&](uint32_t code, int len) {
        acc |= (uint64_t)code << (64 - o - len);
        o += len;
        if (o >= 32) flush();
      };
      code_block(d_codes, zz, info.pred, info.chroma, put);
      if (info.last_of_segment) {                                  // pad the segment's last byte with 1-bits
        const int pad = (8 - (o & 7)) & 7;
        if (pad) put((1u << pad) - 1, pad);
      }
      if (o > 0) flush();
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < nwords; w += 128)
    if (w_first + w < arena_words) arena[w_first + w] = __builtin_bswap32(tile[w]);        // bytes in stream order
}

__device__ __forceinline__ int ff_bytes(uint32_t v) {
  return ((v & 0xffu) == 0xffu) + ((v & 0xff00u) == 0xff00u) + ((v & 0xff0000u) == 0xff0000u) + ((v >> 24) == 0xffu);
}

// grid = the arena's tiles that hold data; one word per lane
__global__ __launch_bounds__(256) void enc_ff_count_kernel(const uint32_t* __restrict__ arena, const int64_t* __restrict__ segword,
                                                           const int64_t* __restrict__ seg0, int n, int32_t* __restrict__ ffcnt) {
  __shared__ int part[4];
  const int64_t words = segword[seg0[n]];
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int c = w < words ? ff_bytes(arena[w]) : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) ffcnt[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// FF bytes of the arena before byte p (p <= the bytes the arena holds)
__device__ __forceinline__ int64_t ff_before(int64_t p, const uint32_t* __restrict__ arena, const int64_t* __restrict__ ffscan) {
  const int64_t t = p / kFfTile;
  int64_t f = ffscan[t];
  const int64_t w1 = p >> 2;
  for (int64_t w = t * (kFfTile / 4); w < w1; ++w) f += ff_bytes(arena[w]);
  if (p & 3) f += ff_bytes(arena[w1] & ((1u << (8 * (p & 3))) - 1u));           // the bytes of that word before p
  return f;
}

// one lane per segment.  file: the segments belong to files (a header in front of an image's first, EOI behind its last)
__global__ __launch_bounds__(256) void enc_sizes_kernel(const Image* __restrict__ images, int n, const int64_t* __restrict__ seg0,
                                                        const int64_t* __restrict__ segword, const int32_t* __restrict__ segbytes,
                                                        const uint32_t* __restrict__ arena, const int64_t* __restrict__ ffscan,
                                                        const int32_t* __restrict__ status, int file, int64_t* __restrict__ segff,
                                                        int64_t* __restrict__ segsize) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= seg0[n]) return;
  const int i = (int)shdr::last_le(seg0, n, s);
  const int64_t p0 = segword[s] * 4;
  const int64_t f0 = ff_before(p0, arena, ffscan), f1 = ff_before(p0 + segbytes[s], arena, ffscan);
  segff[s] = f0;
  int64_t size = segbytes[s] + (f1 - f0);
  if (s + 1 < seg0[i + 1] || file) size += 2;
  if (file && s == seg0[i]) size += header_length(images[i]);
  segsize[s] = status[i] == kOk ? size : 0;
}

// grid = the arena's tiles that hold data; one word per lane.  The bytes a tile writes lie back to back in the output except where it
// crosses an image's header, so they are put together in an LDS window that starts at the tile's first output byte (rounded down to a
// word): every word of the window whose four bytes are all this tile's is stored whole; bytes go out one by one only where a word is
// shared -- the window's two ragged ends, the edge of a header -- or where a tile that spans many small images leaves the window.
__global__ __launch_bounds__(256) void enc_final_kernel(const Image* __restrict__ images, int n, const int64_t* __restrict__ seg0,
                                                        const int64_t* __restrict__ segword, const int32_t* __restrict__ segbytes,
                                                        const uint32_t* __restrict__ arena, const int64_t* __restrict__ ffscan,
                                                        const int64_t* __restrict__ segff, const int64_t* __restrict__ segout,
                                                        const int32_t* __restrict__ status, int file, uint8_t* __restrict__ out,
                                                        int64_t capacity) {
  __shared__ int part[4];
  __shared__ uint32_t stage[kStageWords], owned[kStageWords];      // the window's bytes, and FF in every byte this tile wrote
  __shared__ unsigned long long first_s;                           // the tile's first output byte
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nseg = seg0[n];
  const int64_t words = segword[nseg];
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t v = w < words ? arena[w] : 0u;
  const int mine = ff_bytes(v);
  const int incl = shdr::wave_scan(mine);                          // (not block_scan: the barrier below also covers the cleared window)
  if (lane == 63) part[wave] = incl;
  if (threadIdx.x == 0) first_s = ~0ull;
  for (int k = threadIdx.x; k < kStageWords; k += 256) stage[k] = owned[k] = 0u;
  __syncthreads();
  int64_t f = ffscan[blockIdx.x] + incl - mine;                    // FF bytes of the arena before this word
  for (int k = 0; k < wave; ++k) f += part[k];
  // this lane's segment, its bytes of it, and where the first of them goes
  bool active = w < words;
  int64_t s = 0, j0 = 0, nb = 0, dst = 0;
  int i = 0;
  if (active) {
    s = shdr::last_le(segword, nseg, w);
    i = (int)shdr::last_le(seg0, n, s);
    j0 = (w - segword[s]) * 4;
    nb = segbytes[s];
    active = status[i] == kOk && j0 < nb;                          // (not an image that was refused, not a gap word)
  }
  if (active) {
    dst = segout[s] + j0 + (f - segff[s]);
    if (file && s == seg0[i]) dst += header_length(images[i]);
    atomicMin(&first_s, (unsigned long long)dst);
  }
  __syncthreads();
  if (first_s == ~0ull) return;                                    // (the whole workgroup: nothing of this tile is written)
  const int64_t base = (int64_t)first_s & ~(int64_t)3;
  if (active) {
    auto store = [&](int byte) {
      const int64_t r = dst - base;
      if (dst < capacity) {
        if (r < (int64_t)kStageWords * 4) {
          atomicOr(&stage[r >> 2], (uint32_t)byte << (8 * (int)(r & 3)));
          atomicOr(&owned[r >> 2], 0xffu << (8 * (int)(r & 3)));
        } else {
          out[dst] = (uint8_t)byte;
        }
      }
      ++dst;
    };
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (j0 + k >= nb) break;
      const int byte = (int)((v >> (8 * k)) & 255u);
      store(byte);
      if (byte == 0xFF) store(0);
      if (j0 + k == nb - 1) {                                      // the marker behind the segment
        const bool last = s + 1 == seg0[i + 1];
        if (!last) {
          store(0xFF);
          store(rst_marker(s - seg0[i]));
        } else if (file) {
          store(0xFF);
          store(0xD9);
        }
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kStageWords; k += 256) {
    const uint32_t m = owned[k];
    if (m == 0u) continue;
    const int64_t p = base + 4 * (int64_t)k;
    if (m == 0xffffffffu) {
      *reinterpret_cast<uint32_t*>(out + p) = stage[k];
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if ((m >> (8 * b)) & 1u) out[p + b] = (uint8_t)(stage[k] >> (8 * b));
    }
  }
}

// grid = N + 1: offsets[], and the header of image blockIdx.x
__global__ __launch_bounds__(256) void enc_header_kernel(const Image* __restrict__ images, int n, const int64_t* __restrict__ seg0,
                                                         const int64_t* __restrict__ segout, const int32_t* __restrict__ status,
                                                         const uint8_t* __restrict__ headers, uint8_t* __restrict__ out, int64_t capacity,
                                                         int64_t* __restrict__ offsets) {
  const int i = blockIdx.x;
  const int64_t at = segout[seg0[i]];
  if (threadIdx.x == 0) offsets[i] = at;
  if (i >= n || !headers || status[i] != kOk) return;
  const int len = header_length(images[i]);
  for (int k = threadIdx.x; k < len; k += 256)
    if (at + k < capacity) out[at + k] = headers[(int64_t)i * kHeaderMax + k];
}

int check_images(const char* what, const Image* images, int n, int64_t* blocks, int64_t* segs, int64_t* mcus, int64_t* bound) {
  SHDR_REQUIRE(images, SHDR_E_NULL, "%s: null image table", what);
  SHDR_REQUIRE(n > 0 && n <= kMaxImages, SHDR_E_SHAPE, "%s: the number of images must be 1 .. %d, got %d", what, kMaxImages, n);
  int64_t b = 0, s = 0, m = 0, o = 0;
  for (int i = 0; i < n; ++i) {
    SHDR_REQUIRE(image_ok(images[i]), SHDR_E_SHAPE,
                 "%s: image %d: need H and W in 1 .. 65535, layout 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), quality 1 .. 100 and a restart "
                 "interval 0 .. 65535, got %d x %d, layout %d, quality %d, restart %d", what, i, images[i].height, images[i].width,
                 images[i].layout, images[i].quality, images[i].restart);
    const Geometry g = geometry(images[i]);
    b += g.blocks; s += g.segments; m += g.mcus; o += out_bound(g);
    SHDR_REQUIRE(b <= kMaxBlocks, SHDR_E_SHAPE, "%s: more than %lld blocks in one call", what, (long long)kMaxBlocks);
  }
  *blocks = b; *segs = s; *mcus = m; *bound = o;
  return SHDR_OK;
}

// the passes behind the coefficients; headers_dev NULL: scans only
int entropy_passes(const char* what, const int16_t* coef, const Image* images_dev, const uint8_t* headers_dev, int n, int64_t blocks,
                   int64_t segs, uint8_t* out, int64_t capacity, int64_t* offsets, int32_t* status, const EncWorkspace& w, hipStream_t st,
                   shdr::StageTimer<SHDR_JPEG_ENC_STAGES>& timer) {
  const int file = headers_dev ? 1 : 0;
  const unsigned seg_grid = (unsigned)((segs + 256) / 256);
  // every tile that can hold data: the kernels read how many words do from segword[S]
  const unsigned ff_grid = (unsigned)w.ff_tiles;
  hipLaunchKernelGGL(enc_bits_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, st, coef, images_dev, n, w.blk0, w.seg0, w.bits,
                     status);
  timer.mark();
  hipLaunchKernelGGL(enc_scan_kernel<int32_t>, dim3(1), dim3(1024), 0, st, w.bits, blocks, w.bitpos);
  hipLaunchKernelGGL(enc_segments_kernel, dim3(seg_grid), dim3(256), 0, st, images_dev, n, w.blk0, w.seg0, w.bitpos, w.segword, w.segbytes);
  timer.mark();
  hipLaunchKernelGGL(enc_write_kernel, dim3((unsigned)((blocks + kTileBlocks - 1) / kTileBlocks)), dim3(128), 0, st, coef, images_dev, n,
                     w.blk0, w.seg0, w.bitpos, w.segword, status, w.arena, w.arena_words);
  timer.mark();
  hipLaunchKernelGGL(enc_ff_count_kernel, dim3(ff_grid), dim3(256), 0, st, w.arena, w.segword, w.seg0, n, w.ffcnt);
  hipLaunchKernelGGL(enc_scan_kernel<int32_t>, dim3(1), dim3(1024), 0, st, w.ffcnt, w.ff_tiles, w.ffscan);
  timer.mark();
  hipLaunchKernelGGL(enc_sizes_kernel, dim3(seg_grid), dim3(256), 0, st, images_dev, n, w.seg0, w.segword, w.segbytes, w.arena, w.ffscan,
                     status, file, w.segff, w.segsize);
  hipLaunchKernelGGL(enc_scan_kernel<int64_t>, dim3(1), dim3(1024), 0, st, w.segsize, segs, w.segout);
  timer.mark();
  hipLaunchKernelGGL(enc_final_kernel, dim3(ff_grid), dim3(256), 0, st, images_dev, n, w.seg0, w.segword, w.segbytes, w.arena, w.ffscan,
                     w.segff, w.segout, status, file, out, capacity);
  hipLaunchKernelGGL(enc_header_kernel, dim3((unsigned)n + 1), dim3(256), 0, st, images_dev, n, w.seg0, w.segout, status, headers_dev, out,
                     capacity, offsets);
  timer.mark();
  return shdr::check_launch(what);
}

int check_buffers(const char* what, const void* images_dev, const void* out, const void* offsets, const void* status, const void* workspace) {
  SHDR_REQUIRE(images_dev && out && offsets && status && workspace, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(images_dev) & 3u) == 0, SHDR_E_ALIGN, "%s: images_dev must be 4-byte aligned", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, SHDR_E_ALIGN, "%s: out must be 4-byte aligned", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(offsets) & 7u) == 0, SHDR_E_ALIGN, "%s: offsets must be 8-byte aligned", what);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(status) & 3u) == 0, SHDR_E_ALIGN, "%s: status must be 4-byte aligned", what);
  SHDR_REQUIRE(shdr::aligned16(workspace), SHDR_E_ALIGN, "%s: workspace must be 16-byte aligned", what);
  return SHDR_OK;
}

}  // namespace

extern "C" int shdr_jpeg_encode_batch_sizes(const shdr_jpeg_enc_image* images, int n_images, int64_t* out_bytes, int64_t* n_blocks,
                                            int64_t* workspace_bytes) {
  int64_t blocks = 0, segs = 0, mcus = 0, bound = 0;
  if (int rc = check_images("jpeg_encode_batch_sizes", reinterpret_cast<const Image*>(images), n_images, &blocks, &segs, &mcus, &bound)) return rc;
  if (out_bytes) *out_bytes = bound;
  if (n_blocks) *n_blocks = blocks;
  if (workspace_bytes) *workspace_bytes = carve(nullptr, n_images, blocks, segs).bytes;
  return SHDR_OK;
}

extern "C" int shdr_jpeg_encode_batch(const void* pixels, int pixel_type, const shdr_jpeg_enc_image* images,
                                      const shdr_jpeg_enc_image* images_dev, const uint8_t* headers, const uint8_t* headers_dev, int n_images,
                                      uint8_t* out, int64_t out_capacity, int64_t* offsets, int32_t* status, void* workspace, void* stream,
                                      float* stage_ms) {
  const char* what = "jpeg_encode_batch";
  const Image* im = reinterpret_cast<const Image*>(images);
  const Image* im_dev = reinterpret_cast<const Image*>(images_dev);
  int64_t blocks = 0, segs = 0, mcus = 0, bound = 0;
  if (int rc = check_images(what, im, n_images, &blocks, &segs, &mcus, &bound)) return rc;
  SHDR_REQUIRE(pixels && headers && headers_dev, SHDR_E_NULL, "%s: null pointer", what);
  if (int rc = check_buffers(what, images_dev, out, offsets, status, workspace)) return rc;
  SHDR_REQUIRE(pixel_type == SHDR_JPEG_ENC_U8 || pixel_type == SHDR_JPEG_ENC_F32, SHDR_E_SHAPE, "%s: pixel_type must be 0 (uint8) or 1 (float32), got %d",
               what, pixel_type);
  SHDR_REQUIRE(pixel_type == SHDR_JPEG_ENC_U8 || (reinterpret_cast<uintptr_t>(pixels) & 3u) == 0, SHDR_E_ALIGN, "%s: float pixels must be 4-byte aligned", what);
  SHDR_REQUIRE(out_capacity >= bound, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity, (long long)bound);
  for (int i = 0; i < n_images; ++i) {
    uint8_t want[kHeaderMax];
    const int len = compose_header(im[i], want);
    SHDR_REQUIRE(memcmp(want, headers + (int64_t)i * kHeaderMax, (size_t)len) == 0, SHDR_E_SHAPE,
                 "%s: header %d is not what shdr_jpeg_encode_header_host composes for the image", what, i);
  }
  const EncWorkspace w = carve(workspace, n_images, blocks, segs);
  hipStream_t st = shdr::stream_of(stream);
  shdr::StageTimer<SHDR_JPEG_ENC_STAGES> timer(stage_ms, st);
  hipLaunchKernelGGL(enc_setup_kernel, dim3(1), dim3(64), 0, st, im_dev, n_images, w.mcu0, w.blk0, w.seg0, w.pix0, status);
  if (pixel_type == SHDR_JPEG_ENC_U8)
    hipLaunchKernelGGL(enc_transform_kernel<uint8_t>, dim3((unsigned)mcus), dim3(64), 0, st, static_cast<const uint8_t*>(pixels), im_dev, n_images,
                       w.mcu0, w.blk0, w.pix0, w.coef);
  else
    hipLaunchKernelGGL(enc_transform_kernel<float>, dim3((unsigned)mcus), dim3(64), 0, st, static_cast<const float*>(pixels), im_dev, n_images,
                       w.mcu0, w.blk0, w.pix0, w.coef);
  timer.mark();
  return entropy_passes(what, w.coef, im_dev, headers_dev, n_images, blocks, segs, out, out_capacity, offsets, status, w, st, timer);
}

extern "C" int shdr_jpeg_encode_entropy_batch(const int16_t* coef, int64_t coef_blocks, const shdr_jpeg_enc_image* images,
                                              const shdr_jpeg_enc_image* images_dev, int n_images, uint8_t* out, int64_t out_capacity,
                                              int64_t* offsets, int32_t* status, void* workspace, void* stream, float* stage_ms) {
  const char* what = "jpeg_encode_entropy_batch";
  const Image* im_dev = reinterpret_cast<const Image*>(images_dev);
  int64_t blocks = 0, segs = 0, mcus = 0, bound = 0;
  if (int rc = check_images(what, reinterpret_cast<const Image*>(images), n_images, &blocks, &segs, &mcus, &bound)) return rc;
  SHDR_REQUIRE(coef, SHDR_E_NULL, "%s: null pointer", what);
  if (int rc = check_buffers(what, images_dev, out, offsets, status, workspace)) return rc;
  SHDR_REQUIRE(shdr::aligned16(coef), SHDR_E_ALIGN, "%s: the coefficient arena must be 16-byte aligned", what);
  SHDR_REQUIRE(coef_blocks == blocks, SHDR_E_SHAPE, "%s: the arena holds %lld blocks, the images have %lld", what, (long long)coef_blocks,
               (long long)blocks);
  SHDR_REQUIRE(out_capacity >= bound, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity, (long long)bound);
  const EncWorkspace w = carve(workspace, n_images, blocks, segs);
  hipStream_t st = shdr::stream_of(stream);
  shdr::StageTimer<SHDR_JPEG_ENC_STAGES> timer(stage_ms, st);
  hipLaunchKernelGGL(enc_setup_kernel, dim3(1), dim3(64), 0, st, im_dev, n_images, w.mcu0, w.blk0, w.seg0, w.pix0, status);
  timer.mark();
  return entropy_passes(what, coef, im_dev, nullptr, n_images, blocks, segs, out, out_capacity, offsets, status, w, st, timer);
}
