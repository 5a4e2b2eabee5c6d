// OpenEXR PIZ chunks of a BATCH encoded on the device: the forward rules are those of piz.h, the very code of the host routine
// shdr_piz_encode_host, so the bytes are the same on both sides.  One workgroup per chunk in every per-chunk launch:
//   clear    one memset: the per-chunk histograms, code lengths, table words and the words of the code-word streams
//   front    the presence bitmap in LDS (atomicOr), its popcounts scanned into the forward LUT (rank = before[word] + popcount of the
//            bits below), minNonZero / maxNonZero; then the word planes in strips of P columns (P the largest power of two <=
//            min(width, rows) <= 32; aligned strips never touch each other at any level), four strips at a time: LUT, all levels of the
//            forward wavelet in LDS, the values written in the chunk's value order
//   hist     every lane owns the stretches of equal values that START in its segment of the sequence (a stretch that runs on is
//            followed through the segments' summaries in LDS, not value by value); integer atomicAdd into LDS counters for the 4096
//            values next to 0 and the 4096 next to 65535 (where wavelet coefficients crowd: on smooth images nearly every token is one of
//            a few values, and their atomics on one address in memory were the whole stage), into the chunk's histogram for the rest
//   code     works from the used-symbol bitmap that hist leaves (no pass visits the unused symbols): the used symbols compacted in
//            symbol order, a stable LSD radix sort by count (4 bits a pass: (count, symbol) order),
//            the two-queue merge by ONE lane (weights in LDS up to kLdsSyms symbols, else in the workspace), depths by every leaf
//            walking to the root, canonical codes by a counting sort over lengths (the decoder's), the packed table from the closed
//            form of the zero stretch in front of every used symbol
//   bits     token bit lengths per lane, a scan, the chunk's size and whether it is coded; then the code words, each lane gathering
//            its bits into 32-bit words that are OR-ed into the cleared stream (integer OR: the order of arrival does not matter)
//   scan     out_offsets from the stored sizes (scan_array of batch.h, as the deflate encoders)
//   final    the chunk's bytes at their final place: header, bitmap, block header, table, code words -- or the scanline bytes
// Stream-ordered, no host wait, no allocation, integer atomics only: the same input gives the same bytes.
#include "shdr_internal.h"
#include "batch.h"
#include "piz.h"

namespace {

using namespace shdr_piz;

constexpr int kWide = 1024;                                      // lanes of front, hist and bits
constexpr int kCodeThreads = 512;
constexpr int kRankLanes = 256;                                  // lanes of the counting sort over lengths
constexpr int kCopyThreads = 256;
constexpr int kSymPad = 65600;                                   // kSymbols rounded up
constexpr int kNear = 4096;                                      // values next to 0 and next to 65535 counted in LDS by hist
constexpr int kLdsSyms = 2048;                                   // used symbols up to which the merge's weights live in LDS
constexpr int kWordsPerCodeLane = kBitmapWords / kCodeThreads;   // words of the used-symbol bitmap per lane of code: 4
constexpr int kWordsPerRankLane = kBitmapWords / kRankLanes;     // ... per lane of its counting sort: 8
constexpr int64_t kTableBytes = ((6 * (int64_t)kSymbols + 7) / 8 + 4 + 15) & ~(int64_t)15;
constexpr int64_t kZeroBytes = 4 * (int64_t)kSymPad + kSymPad + kTableBytes;     // per chunk: hist, lens, table
static_assert(kZeroBytes % 16 == 0, "per-chunk regions keep 16-byte alignment");

using shdr::block_scan;

struct Meta {                                 // what the launches hand over, per chunk
  uint32_t ok, bm_min, bm_max, max_value, im, iM, runs, table_bits;
  uint64_t n_bits;
  int64_t size;
  uint32_t coded, n_used, merge_ticks, pad_;
};
static_assert(sizeof(Meta) == 64, "Meta is 64 bytes");

struct Ws {                                   // carved out of the caller's workspace, every part 16-byte aligned
  uint8_t* zero;                              // [C][kZeroBytes], then the code-word streams: cleared in front of every call
  uint8_t* data;                              // [total + 8 C + 8]
  int64_t zero_bytes;
  Meta* meta;                                 // [C]
  uint32_t* bitmap;                           // [C][kBitmapWords] as stored (bit 0 clear)
  uint32_t* used;                             // [C][kBitmapWords] the symbols 0 .. 65535 that the chunk's code has
  uint64_t* keys_a;                           // [C][kSymPad]
  uint64_t* keys_b;                           // [C][kSymPad] the sort's other buffer, then the code of every symbol
  uint32_t* parent;                           // [C][2 kSymPad]
  uint32_t* weight;                           // [C][kSymPad]
  uint32_t* made;                             // [C][kSymPad]
  uint16_t* vals;                             // [total / 2]
  int64_t* sizes;                             // [C]
  int64_t bytes;
  __host__ __device__ uint32_t* hist(int64_t c) const { return reinterpret_cast<uint32_t*>(zero + c * kZeroBytes); }
  __host__ __device__ uint8_t* lens(int64_t c) const { return zero + c * kZeroBytes + 4 * (int64_t)kSymPad; }
  __host__ __device__ uint32_t* table(int64_t c) const { return reinterpret_cast<uint32_t*>(zero + c * kZeroBytes + 5 * (int64_t)kSymPad); }
  // the words of chunk c's code words: word-aligned, with room for the chunk's bytes and a word more
  __host__ __device__ uint32_t* stream(int64_t c, int64_t lo) const { return reinterpret_cast<uint32_t*>(data + ((lo + 3) & ~(int64_t)3) + 8 * c); }
};
Ws carve(void* base, int64_t c, int64_t total) {
  Ws w;
  shdr::Carver cut(base);
  w.zero = cut.take<uint8_t>(c * kZeroBytes);                    // a multiple of 16: data follows at once, and ONE clear
  w.data = cut.take<uint8_t>(total + 8 * c + 8);                 // of zero_bytes covers both
  w.zero_bytes = cut.bytes();
  w.meta = cut.take<Meta>(c);
  w.bitmap = cut.take<uint32_t>((int64_t)kBitmapWords * c);
  w.used = cut.take<uint32_t>((int64_t)kBitmapWords * c);
  w.keys_a = cut.take<uint64_t>((int64_t)kSymPad * c);
  w.keys_b = cut.take<uint64_t>((int64_t)kSymPad * c);
  w.parent = cut.take<uint32_t>(2 * (int64_t)kSymPad * c);
  w.weight = cut.take<uint32_t>((int64_t)kSymPad * c);
  w.made = cut.take<uint32_t>((int64_t)kSymPad * c);
  w.vals = cut.take<uint16_t>((total + 1) / 2);
  w.sizes = cut.take<int64_t>(c);
  w.bytes = cut.bytes();
  return w;
}

struct Tables {                               // the batch's tables on the device
  const int64_t* chunk_off;
  const int32_t* geom;
  const int32_t* chan_words;
  int64_t total;
  int n_words;
};

struct Chunk {
  int64_t lo, n;                              // the scanline bytes
  uint32_t nv;                                // values
  int width, rows, n_chan;
  const int32_t* cw;
  bool ok;
};
__device__ __forceinline__ Chunk chunk_of(const Tables& tb, int64_t c) {
  Chunk k;
  const shdr::Span span = shdr::clamped_span(tb.chunk_off, c, tb.total);
  k.lo = span.lo;
  k.n = span.n;
  k.width = tb.geom[4 * c];
  k.rows = tb.geom[4 * c + 1];
  const int first = tb.geom[4 * c + 2];
  k.n_chan = tb.geom[4 * c + 3];
  k.cw = tb.chan_words + (first >= 0 ? first : 0);
  int64_t values = 0;
  if (first >= 0 && k.n_chan >= 1 && (int64_t)first + k.n_chan <= tb.n_words) values = chunk_values(k.width, k.rows, k.cw, k.n_chan);
  k.nv = (uint32_t)values;
  k.ok = values > 0 && 2 * values == k.n && (k.lo & 1) == 0;     // (never false with the tables the host checked)
  return k;
}

// The stretches of equal elements of v[0 .. n), cut into one segment per lane.  summary: what a segment starts with and how many
// of its leading elements equal that (LDS, one entry per lane; a barrier follows).  walk: f(value, L) for every stretch that STARTS in
// this lane's segment, in order; a stretch that reaches the segment's end is followed through the summaries.
template <int THREADS>
struct Segments {
  uint32_t n, per, s0, s1;
  __device__ __forceinline__ Segments(uint32_t n_) : n(n_) {
    per = (n + THREADS - 1) / THREADS;
    s0 = lo(threadIdx.x);
    s1 = lo(threadIdx.x + 1);
  }
  __device__ __forceinline__ uint32_t lo(uint32_t t) const { return t * per < n ? t * per : n; }
  template <class E>
  __device__ __forceinline__ void summary(const E* v, uint16_t* s_first, uint32_t* s_lead) const {
    uint32_t first = 0, lead = 0;
    if (s0 < s1) {
      first = v[s0];
      lead = 1;
      while (s0 + lead < s1 && v[s0 + lead] == first) ++lead;
    }
    s_first[threadIdx.x] = (uint16_t)first;
    s_lead[threadIdx.x] = lead;
    __syncthreads();
  }
  template <class E, class F>
  __device__ __forceinline__ void walk(const E* v, const uint16_t* s_first, const uint32_t* s_lead, F&& f) const {
    uint32_t i = s0;
    if (i < s1 && i > 0 && v[i - 1] == v[i]) i += s_lead[threadIdx.x];   // the leading stretch started earlier
    while (i < s1) {
      const uint32_t val = v[i];
      uint32_t j = i + 1;
      while (j < s1 && v[j] == val) ++j;
      uint32_t L = j - i;
      if (j == s1) {
        for (uint32_t u = threadIdx.x + 1; u < (uint32_t)THREADS; ++u) {
          const uint32_t len = lo(u + 1) - lo(u);
          if (!len || s_first[u] != val) break;
          L += s_lead[u];
          if (s_lead[u] < len) break;
        }
      }
      f(val, L);
      i = j;
    }
  }
};

struct DevOut {
  uint32_t* p;
  __device__ __forceinline__ void word(int64_t i, uint32_t w) const {
    if (w) atomicOr(p + i, __builtin_bswap32(w));
  }
};

// ---- front: bitmap, LUT, wavelet ----------------------------------------------------------------------------------------------------
template <bool W14>
__device__ __forceinline__ void enc_level(uint16_t (*tile)[kMaxRows + 1], int w, int ny, int p, int p2, int t) {
  const int bx = w >= p2 ? (w - p2) / p2 + 1 : 0, by = ny >= p2 ? (ny - p2) / p2 + 1 : 0;      // whole blocks
  const int xs = bx * p2, ys = by * p2;                          // where the loops stop
  const int colx = (w & p) ? 1 : 0, rowy = (ny & p) ? 1 : 0;
  const int items = by * (bx + colx) + rowy * bx;
  for (int i = t; i < items; i += 256) {
    if (i < by * (bx + colx)) {
      const int y = (i / (bx + colx)) * p2, k = i % (bx + colx);
      if (k < bx) {
        const int x = k * p2;
        enc_quad<W14>(tile[y][x], tile[y][x + p], tile[y + p][x], tile[y + p][x + p]);
      } else {
        enc<W14>(tile[y][xs], tile[y + p][xs], tile[y][xs], tile[y + p][xs]);
      }
    } else {
      const int x = (i - by * (bx + colx)) * p2;
      enc<W14>(tile[ys][x], tile[ys][x + p], tile[ys][x], tile[ys][x + p]);
    }
  }
}

__global__ __launch_bounds__(kWide) void piz_enc_front_kernel(const uint8_t* __restrict__ planar, Tables tb, Ws ws) {
  __shared__ uint32_t words[kBitmapWords];
  __shared__ uint32_t before[kBitmapWords];
  __shared__ uint16_t tile[4][kMaxRows][kMaxRows + 1];
  __shared__ int part[kWide / 64];
  __shared__ uint32_t s_lo, s_hi;
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  const Chunk k = chunk_of(tb, c);
  Meta* meta = ws.meta + c;
  if (!k.ok) {
    if (t == 0) meta->ok = 0;
    return;
  }
  const uint16_t* raw = reinterpret_cast<const uint16_t*>(planar + k.lo);
  words[2 * t] = 0;
  words[2 * t + 1] = 0;
  if (t == 0) {
    s_lo = kBitmapBytes - 1;
    s_hi = 0;
  }
  __syncthreads();
  for (uint32_t i = t; i < k.nv; i += kWide) {
    const uint32_t v = raw[i];
    atomicOr(&words[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  uint32_t w0 = words[2 * t], w1 = words[2 * t + 1];
  if (t == 0) w0 &= ~1u;                                         // value 0 is implied
  ws.bitmap[c * kBitmapWords + 2 * t] = w0;
  ws.bitmap[c * kBitmapWords + 2 * t + 1] = w1;
  if (w0 | w1) {
    const uint32_t low = w0 ? 8u * t + ((uint32_t)__builtin_ctz(w0) >> 3) : 8u * t + 4u + ((uint32_t)__builtin_ctz(w1) >> 3);
    const uint32_t high = w1 ? 8u * t + 4u + ((31u - (uint32_t)__builtin_clz(w1)) >> 3) : 8u * t + ((31u - (uint32_t)__builtin_clz(w0)) >> 3);
    atomicMin(&s_lo, low);
    atomicMax(&s_hi, high);
  }
  if (t == 0) {
    w0 |= 1u;
    words[0] = w0;
  }
  int present = 0;
  const int mine = __builtin_popcount(w0) + __builtin_popcount(w1);
  const int excl = block_scan<kWide>(mine, part, present);
  before[2 * t] = (uint32_t)excl;
  before[2 * t + 1] = (uint32_t)(excl + __builtin_popcount(w0));
  __syncthreads();
  const uint32_t max_value = (uint32_t)present - 1;
  if (t == 0) {
    meta->ok = 1;
    meta->bm_min = s_lo;
    meta->bm_max = s_hi;
    meta->max_value = max_value;
  }
  const bool w14 = max_value < 16384u;
  const int nx = k.width, ny = k.rows;
  const int P = top_power(nx < ny ? nx : ny);
  const int64_t strips = (nx + P - 1) / P;
  int64_t row_words = 0, planes = 0;
  for (int ch = 0; ch < k.n_chan; ++ch) {
    row_words += (int64_t)nx * k.cw[ch];
    planes += k.cw[ch];
  }
  const int64_t tiles = planes * strips;
  uint16_t* vals = ws.vals + k.lo / 2;
  const int g = t >> 8, lt = t & 255;
  for (int64_t base = 0; base < tiles; base += 4) {
    const int64_t tl = base + g;
    const bool active = tl < tiles;
    int words_ = 1, j = 0, x0 = 0, w = 0;
    int64_t value_at = 0, row_at = 0;
    if (active) {
      int plane = (int)(tl / strips), ch = 0;
      x0 = (int)(tl % strips) * P;
      w = nx - x0 < P ? nx - x0 : P;
      for (; ch < k.n_chan - 1 && plane >= k.cw[ch]; ++ch) {
        plane -= k.cw[ch];
        value_at += (int64_t)nx * ny * k.cw[ch];
        row_at += (int64_t)nx * k.cw[ch];
      }
      words_ = k.cw[ch];
      j = plane;
      for (int i = lt; i < ny * w; i += 256) {
        const int y = i / w, x = i % w;
        tile[g][y][x] = (uint16_t)lut_rank(words, before, raw[(int64_t)y * row_words + row_at + (int64_t)(x0 + x) * words_ + j]);
      }
    }
    __syncthreads();
    for (int p = 1, p2 = 2; p2 <= P; p = p2, p2 <<= 1) {
      if (active) {
        if (w14) enc_level<true>(tile[g], w, ny, p, p2, lt);
        else enc_level<false>(tile[g], w, ny, p, p2, lt);
      }
      __syncthreads();
    }
    if (active) {
      for (int i = lt; i < ny * w; i += 256) {
        const int y = i / w, x = i % w;
        vals[value_at + ((int64_t)y * nx + x0 + x) * words_ + j] = tile[g][y][x];
      }
    }
    __syncthreads();
  }
}

// ---- hist: the tokens' frequencies --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWide) void piz_enc_hist_kernel(Tables tb, Ws ws) {
  __shared__ uint16_t s_first[kWide];
  __shared__ uint32_t s_lead[kWide];
  __shared__ uint32_t s_runs, s_min, s_max;
  __shared__ uint32_t s_near[2 * kNear];                         // counts of the values 0 .. kNear - 1 and 65536 - kNear .. 65535
  __shared__ uint32_t s_used[kBitmapWords];                      // the values that are tokens (and the run code, if below 65536)
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  Meta* meta = ws.meta + c;
  if (!meta->ok) return;
  const Chunk k = chunk_of(tb, c);
  const uint16_t* vals = ws.vals + k.lo / 2;
  uint32_t* hist = ws.hist(c);
  for (int i = t; i < 2 * kNear; i += kWide) s_near[i] = 0;
  for (int i = t; i < kBitmapWords; i += kWide) s_used[i] = 0;
  if (t == 0) {
    s_runs = 0;
    s_min = 65535;
    s_max = 0;
  }
  const Segments<kWide> seg(k.nv);
  seg.summary(vals, s_first, s_lead);
  uint32_t my_runs = 0, mn = 65535, mx = 0;
  seg.walk(vals, s_first, s_lead, [&](uint32_t val, uint32_t L) {
    uint32_t lit, runs;
    stretch_tokens(L, lit, runs);
    if (val < (uint32_t)kNear) atomicAdd(&s_near[val], lit);
    else if (val >= 65536u - kNear) atomicAdd(&s_near[val - (65536u - 2 * kNear)], lit);
    else atomicAdd(&hist[val], lit);
    const uint32_t bit = 1u << (val & 31);                       // (a stale read only costs an atomic that changes nothing)
    if (!(const_cast<volatile uint32_t*>(s_used)[val >> 5] & bit)) atomicOr(&s_used[val >> 5], bit);
    my_runs += runs;
    mn = val < mn ? val : mn;
    mx = val > mx ? val : mx;
  });
  if (my_runs) atomicAdd(&s_runs, my_runs);
  if (mn <= mx) {
    atomicMin(&s_min, mn);
    atomicMax(&s_max, mx);
  }
  __syncthreads();
  for (int i = t; i < 2 * kNear; i += kWide)                     // (nothing else touches these entries of the cleared histogram)
    if (const uint32_t n = s_near[i]) hist[i < kNear ? i : i + (65536 - 2 * kNear)] = n;
  if (t == 0) {
    meta->im = s_min;
    meta->iM = s_max + 1;
    meta->runs = s_runs;
    hist[s_max + 1] = 1 + s_runs;                                // no value is iM: the run code's count is stored, not added
    if (s_max + 1 < 65536u) s_used[(s_max + 1) >> 5] |= 1u << ((s_max + 1) & 31);
  }
  __syncthreads();
  for (int i = t; i < kBitmapWords; i += kWide) ws.used[c * kBitmapWords + i] = s_used[i];
}

// ---- code: sort, merge, depths, canonical codes, table ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kCodeThreads) void piz_enc_code_kernel(Ws ws) {
  __shared__ uint32_t s_radix[16 * kCodeThreads];                // [digit][lane]; later uint16 [length][rank lane]
  __shared__ uint32_t s_weight[kLdsSyms], s_made[kLdsSyms];
  __shared__ uint32_t s_used[kBitmapWords];
  __shared__ Canon canon;
  __shared__ int part[kCodeThreads / 64];
  __shared__ uint32_t s_max;
  __shared__ int s_last[kCodeThreads];                           // the largest used symbol among the lane's words, or -1
  static_assert((kMaxLen + 1) * kRankLanes * 2 <= 16 * kCodeThreads * 4, "the length counters fit the radix counters' LDS");
  static_assert(kWordsPerCodeLane * kCodeThreads == kBitmapWords && kWordsPerRankLane * kRankLanes == kBitmapWords, "lanes share the bitmap");
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  Meta* meta = ws.meta + c;
  if (!meta->ok) return;
  const uint32_t* hist = ws.hist(c);
  uint8_t* lens = ws.lens(c);
  uint64_t* src = ws.keys_a + c * kSymPad;
  uint64_t* dst = ws.keys_b + c * kSymPad;
  const uint32_t im = meta->im, iM = meta->iM;
  const bool top = iM == (uint32_t)kSymbols - 1;                 // the run code 65536 lies beyond the bitmap: it is the last symbol
  for (int i = t; i < kBitmapWords; i += kCodeThreads) s_used[i] = ws.used[c * kBitmapWords + i];
  if (t == 0) s_max = 0;
  __syncthreads();
  // the used symbols in symbol order: key = count << 17 | symbol.  Lane t owns the bitmap words kWordsPerCodeLane t ..
  uint32_t w[kWordsPerCodeLane];
  int mine = 0, last = -1;
#pragma unroll
  for (int k = 0; k < kWordsPerCodeLane; ++k) {
    w[k] = s_used[kWordsPerCodeLane * t + k];
    mine += __builtin_popcount(w[k]);
    if (w[k]) last = 32 * (kWordsPerCodeLane * t + k) + 31 - __builtin_clz(w[k]);
  }
  s_last[t] = last;
  int in_bitmap = 0;
  int at = block_scan<kCodeThreads>(mine, part, in_bitmap);
  const uint32_t n = (uint32_t)in_bitmap + (top ? 1u : 0u);      // >= 2: a value and the run code
  uint32_t most = 0;
#pragma unroll
  for (int k = 0; k < kWordsPerCodeLane; ++k)
    for (uint32_t v = w[k]; v; v &= v - 1) {
      const uint32_t s = 32u * (kWordsPerCodeLane * t + k) + (uint32_t)__builtin_ctz(v), h = hist[s];
      src[at++] = ((uint64_t)h << 17) | s;
      most = h > most ? h : most;
    }
  if (top && t == kCodeThreads - 1) {
    const uint32_t h = hist[kSymbols - 1];
    src[n - 1] = ((uint64_t)h << 17) | (uint32_t)(kSymbols - 1);
    most = h > most ? h : most;
  }
  atomicMax(&s_max, most);
  __syncthreads();
  int passes = (32 - __builtin_clz(s_max | 1u) + 3) / 4;
  passes += passes & 1;                                          // an even number: the sorted keys end in keys_a
  const uint32_t per = (n + kCodeThreads - 1) / kCodeThreads;
  const uint32_t e0 = t * per < n ? t * per : n, e1 = e0 + per < n ? e0 + per : n;
  for (int pass = 0; pass < passes; ++pass) {
    const int shift = 17 + 4 * pass;
    for (int d = 0; d < 16; ++d) s_radix[d * kCodeThreads + t] = 0;
    for (uint32_t e = e0; e < e1; ++e) ++s_radix[(int)((src[e] >> shift) & 15) * kCodeThreads + t];
    __syncthreads();
    int sum = 0;
    for (int i = 0; i < 16; ++i) sum += (int)s_radix[16 * t + i];
    int all = 0;
    int run = block_scan<kCodeThreads>(sum, part, all);
    for (int i = 0; i < 16; ++i) {
      const int x = (int)s_radix[16 * t + i];
      s_radix[16 * t + i] = (uint32_t)run;
      run += x;
    }
    __syncthreads();
    for (uint32_t e = e0; e < e1; ++e) {
      const uint64_t key = src[e];
      dst[s_radix[(int)((key >> shift) & 15) * kCodeThreads + t]++] = key;
    }
    __syncthreads();
    uint64_t* x = src;
    src = dst;
    dst = x;
  }
  // the merge: one lane, a chain of n - 1 steps
  uint32_t* weight = n <= (uint32_t)kLdsSyms ? s_weight : ws.weight + c * kSymPad;
  uint32_t* made = n <= (uint32_t)kLdsSyms ? s_made : ws.made + c * kSymPad;
  uint32_t* parent = ws.parent + c * 2 * (int64_t)kSymPad;
  for (uint32_t i = t; i < n; i += kCodeThreads) weight[i] = (uint32_t)(src[i] >> 17);
  __syncthreads();
  if (t == 0) {
    const uint64_t t0 = wall_clock64();
    huff_merge(weight, n, made, parent);
    meta->n_used = n;
    meta->merge_ticks = (uint32_t)(wall_clock64() - t0);         // measurement (stats): the constant-rate counter
  }
  __syncthreads();
  for (uint32_t i = t; i < n; i += kCodeThreads) lens[src[i] & 0x1FFFFu] = (uint8_t)huff_depth(parent, n, i);
  // canonical codes: a counting sort over lengths, lane r < kRankLanes owns the bitmap words kWordsPerRankLane r .. and column r of cnt
  uint16_t* cnt = reinterpret_cast<uint16_t*>(s_radix);
  for (int i = t; i < (kMaxLen + 1) * kRankLanes; i += kCodeThreads) cnt[i] = 0;
  __syncthreads();
  if (t < kRankLanes)
    for (int k = 0; k < kWordsPerRankLane; ++k)
      for (uint32_t v = s_used[kWordsPerRankLane * t + k]; v; v &= v - 1)
        ++cnt[(int)lens[32 * (kWordsPerRankLane * t + k) + __builtin_ctz(v)] * kRankLanes + t];
  __syncthreads();
  if (t >= 1 && t <= kMaxLen) {
    uint32_t run = 0;
    for (int i = 0; i < kRankLanes; ++i) {
      const uint32_t x = cnt[t * kRankLanes + i];
      cnt[t * kRankLanes + i] = (uint16_t)run;                   // the symbols before lane i's: at most 65535 where it is used
      run += x;
    }
    if (top && lens[kSymbols - 1] == t) ++run;                   // the run code beyond the bitmap: the last symbol of its length
    canon.count[t] = run;
  }
  __syncthreads();
  if (t == 0) make_canon(canon);                                 // (a Huffman code is never over-subscribed)
  __syncthreads();
  uint64_t* code = dst;                                          // keys_b: free since the last pass
  if (t < kRankLanes)
    for (int k = 0; k < kWordsPerRankLane; ++k)
      for (uint32_t v = s_used[kWordsPerRankLane * t + k]; v; v &= v - 1) {
        const int s = 32 * (kWordsPerRankLane * t + k) + __builtin_ctz(v), l = lens[s];
        code[s] = canon.first[l] + (uint32_t)cnt[l * kRankLanes + t]++;
      }
  if (top && t == 0) {
    const int l = lens[kSymbols - 1];
    code[kSymbols - 1] = canon.first[l] + canon.count[l] - 1;
  }
  // the table of the lengths of im .. iM: per used symbol the zero lengths since the one before it, then its own length
  int prev = -1;
  for (int u = t - 1; u >= 0 && prev < 0; --u) prev = s_last[u];
  if (prev < 0) prev = (int)im - 1;                              // (no used symbol lies below im)
  int bits = 0, p = prev;
#pragma unroll
  for (int k = 0; k < kWordsPerCodeLane; ++k)
    for (uint32_t v = w[k]; v; v &= v - 1) {
      const int s = 32 * (kWordsPerCodeLane * t + k) + __builtin_ctz(v);
      bits += (int)table_stretch_bits(0, (uint32_t)(s - p - 1)) + 6;
      p = s;
    }
  if (top && t == kCodeThreads - 1) bits += (int)table_stretch_bits(0, (uint32_t)(kSymbols - 1 - p - 1)) + 6;
  int table_bits = 0;
  const int bit0 = block_scan<kCodeThreads>(bits, part, table_bits);
  BitSink<DevOut> sink(DevOut{ws.table(c)}, (uint64_t)bit0);
  p = prev;
#pragma unroll
  for (int k = 0; k < kWordsPerCodeLane; ++k)
    for (uint32_t v = w[k]; v; v &= v - 1) {
      const int s = 32 * (kWordsPerCodeLane * t + k) + __builtin_ctz(v);
      put_table_stretch(sink, 0, (uint32_t)(s - p - 1));
      sink.put(lens[s], 6);
      p = s;
    }
  if (top && t == kCodeThreads - 1) {
    put_table_stretch(sink, 0, (uint32_t)(kSymbols - 1 - p - 1));
    sink.put(lens[kSymbols - 1], 6);
  }
  sink.flush();
  if (t == 0) meta->table_bits = (uint32_t)table_bits;
}

// ---- bits: sizes and code words -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWide) void piz_enc_bits_kernel(Tables tb, Ws ws, int pad, uint8_t* __restrict__ coded) {
  __shared__ uint16_t s_first[kWide];
  __shared__ uint32_t s_lead[kWide];
  __shared__ int64_t part[kWide / 64];
  __shared__ int s_coded;
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  Meta* meta = ws.meta + c;
  const Chunk k = chunk_of(tb, c);
  if (!meta->ok) {
    if (t == 0) {
      ws.sizes[c] = pad + k.n;
      coded[c] = 0;
      meta->coded = 0;
    }
    return;
  }
  const uint16_t* vals = ws.vals + k.lo / 2;
  const uint8_t* lens = ws.lens(c);
  const uint64_t* code = ws.keys_b + c * kSymPad;
  const uint32_t iM = meta->iM, run_len = lens[iM];
  const uint64_t run_code = code[iM];
  const Segments<kWide> seg(k.nv);
  seg.summary(vals, s_first, s_lead);
  int64_t bits = 0;
  seg.walk(vals, s_first, s_lead, [&](uint32_t val, uint32_t L) { bits += (int64_t)stretch_bits(L, lens[val], run_len); });
  int64_t n_bits = 0;
  const int64_t bit0 = block_scan<kWide>(bits, part, n_bits);
  if (t == 0) {
    const int64_t bm = meta->bm_min <= meta->bm_max ? (int64_t)(meta->bm_max - meta->bm_min + 1) : 0;
    const int64_t size = 4 + bm + 4 + 20 + (int64_t)((meta->table_bits + 7) >> 3) + ((n_bits + 7) >> 3);
    const int use = size < k.n ? 1 : 0;                          // stored as PIZ only where that is strictly smaller
    meta->n_bits = (uint64_t)n_bits;
    meta->size = size;
    meta->coded = (uint32_t)use;
    ws.sizes[c] = pad + (use ? size : k.n);
    coded[c] = (uint8_t)use;
    s_coded = use;
  }
  __syncthreads();
  if (!s_coded) return;
  BitSink<DevOut> sink(DevOut{ws.stream(c, k.lo)}, (uint64_t)bit0);
  seg.walk(vals, s_first, s_lead,
           [&](uint32_t val, uint32_t L) { put_stretch(sink, L, code[val], (uint32_t)lens[val], run_code, run_len); });
  sink.flush();
}

// ---- final: the bytes at their place ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCopyThreads) void piz_enc_final_kernel(const uint8_t* __restrict__ planar, Tables tb, Ws ws, int pad,
                                                                     const int64_t* __restrict__ out_offsets, uint8_t* __restrict__ out,
                                                                     int64_t capacity, int32_t* __restrict__ stats) {
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  const Chunk k = chunk_of(tb, c);
  const Meta* meta = ws.meta + c;
  if (stats && t == 0) {
    stats[SHDR_PIZ_ENC_STATS * c] = meta->ok ? (int32_t)meta->n_used : 0;
    stats[SHDR_PIZ_ENC_STATS * c + 1] = meta->ok ? (int32_t)meta->merge_ticks : 0;
  }
  const int64_t at = out_offsets[c] + pad, end = out_offsets[c + 1];
  if (at < 0 || end > capacity || end < at) return;              // never with the sizes the host checked
  uint8_t* dst = out + at;
  const int64_t room = end - at;
  if (!meta->coded) {
    const uint8_t* src = planar + k.lo;
    for (int64_t i = t; i < k.n && i < room; i += kCopyThreads) dst[i] = src[i];
    return;
  }
  if (meta->size != room) return;                                // (the bits kernel stored both)
  const uint32_t lo = meta->bm_min, hi = meta->bm_max;
  const int64_t bm = lo <= hi ? (int64_t)(hi - lo + 1) : 0;
  const int64_t table_bytes = (meta->table_bits + 7) >> 3, data_bytes = (int64_t)((meta->n_bits + 7) >> 3);
  if (t < 24 + 4) {
    const uint32_t head[7] = {lo | (hi << 16), (uint32_t)(20 + table_bytes + data_bytes), meta->im, meta->iM, (uint32_t)table_bytes,
                              (uint32_t)meta->n_bits, 0u};
    const int f = t >> 2;
    dst[(f ? 4 + bm : 0) + 4 * (f ? f - 1 : 0) + (t & 3)] = (uint8_t)(head[f] >> (8 * (t & 3)));
  }
  const uint32_t* bitmap = ws.bitmap + c * kBitmapWords;
  for (int64_t i = t; i < bm; i += kCopyThreads) {
    const uint32_t b = lo + (uint32_t)i;
    dst[4 + i] = (uint8_t)(bitmap[b >> 2] >> (8 * (b & 3)));
  }
  uint8_t* p = dst + 4 + bm + 24;
  const uint8_t* table = reinterpret_cast<const uint8_t*>(ws.table(c));
  for (int64_t i = t; i < table_bytes; i += kCopyThreads) p[i] = table[i];
  p += table_bytes;
  const uint8_t* data = reinterpret_cast<const uint8_t*>(ws.stream(c, k.lo));
  for (int64_t i = t; i < data_bytes; i += kCopyThreads) p[i] = data[i];
}

// ---- scan: out_offsets[c] = sum of the stored sizes before c, out_offsets[C] = the total.  One block. -------------------------------
__global__ __launch_bounds__(1024) void piz_enc_scan_kernel(const int64_t* __restrict__ sizes, int64_t count, int64_t* __restrict__ out_offsets) {
  const int64_t all = shdr::scan_array<1024, 1>(
      count, [&](int64_t c) { return sizes[c]; }, [&](int64_t c, int64_t before) { out_offsets[c] = before; });
  if (threadIdx.x == 0) out_offsets[count] = all;
}

struct Plan {
  int64_t total, out_bytes, ws_bytes;
};

int make_plan(const char* what, const int64_t* chunk_off, const int32_t* geom, const int32_t* chan_words, int n_words, int n_chunks, int pad,
              Plan& p) {
  SHDR_REQUIRE(chunk_off && geom && chan_words, SHDR_E_NULL, "%s: null table", what);
  SHDR_REQUIRE(n_chunks > 0 && n_words > 0, SHDR_E_SHAPE, "%s: the numbers of chunks and channel words must be positive, got %d and %d", what,
               n_chunks, n_words);
  SHDR_REQUIRE(pad >= 0 && pad <= 4096, SHDR_E_SHAPE, "%s: pad must be in [0, 4096], got %d", what, pad);
  SHDR_REQUIRE(chunk_off[0] == 0, SHDR_E_SHAPE, "%s: chunk_off[0] must be 0", what);
  for (int c = 0; c < n_chunks; ++c) {
    const int32_t* g = geom + 4 * c;
    SHDR_REQUIRE(g[2] >= 0 && g[3] >= 1 && (int64_t)g[2] + g[3] <= n_words, SHDR_E_SHAPE,
                 "%s: chunk %d: channels %d .. %d + %d lie outside the table of %d", what, c, g[2], g[2], g[3], n_words);
    const int64_t values = chunk_values(g[0], g[1], chan_words + g[2], g[3]);
    SHDR_REQUIRE(values > 0, SHDR_E_SHAPE,
                 "%s: chunk %d: width %d, rows %d, %d channels (1 .. 32 rows, 1 .. 64 channels of 1 or 2 words, at most 2^28 bytes)", what, c,
                 g[0], g[1], g[3]);
    SHDR_REQUIRE(chunk_off[c + 1] - chunk_off[c] == 2 * values, SHDR_E_SHAPE, "%s: chunk %d has %lld bytes, its shape holds %lld", what, c,
                 (long long)(chunk_off[c + 1] - chunk_off[c]), (long long)(2 * values));
  }
  p.total = chunk_off[n_chunks];
  p.out_bytes = p.total + (int64_t)pad * n_chunks;               // a stored chunk is never larger than the chunk
  p.ws_bytes = carve(nullptr, n_chunks, p.total).bytes;
  return SHDR_OK;
}

}  // namespace

extern "C" int shdr_piz_wavelet_pair(int which, unsigned a, unsigned b, uint16_t* out) {
  SHDR_REQUIRE(out, SHDR_E_NULL, "piz_wavelet_pair: null pointer");
  SHDR_REQUIRE(which >= 0 && which <= 3, SHDR_E_SHAPE, "piz_wavelet_pair: which must be 0 .. 3 (enc14, enc16, dec14, dec16), got %d", which);
  const uint16_t x = (uint16_t)a, y = (uint16_t)b;
  if (which == 0) enc14(x, y, out[0], out[1]);
  else if (which == 1) enc16(x, y, out[0], out[1]);
  else if (which == 2) dec14(x, y, out[0], out[1]);
  else dec16(x, y, out[0], out[1]);
  return SHDR_OK;
}

extern "C" int64_t shdr_piz_encode_bound(int width, int rows, const int32_t* chan_words, int n_chan) {
  const int64_t values = chunk_values(width, rows, chan_words, n_chan);
  if (values <= 0) {
    shdr::set_error("piz_encode_bound: a shape out of range (1 .. 32 rows, 1 .. 64 channels of 1 or 2 words, at most 2^28 bytes)");
    return -1;
  }
  return encode_bound(values);
}

extern "C" int shdr_piz_encode_host(const uint8_t* raw, int64_t n, int width, int rows, const int32_t* chan_words, int n_chan, uint8_t* dst,
                                    int64_t capacity, int64_t* written) {
  const char* what = "piz_encode_host";
  SHDR_REQUIRE(raw && dst && written && chan_words, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(rows >= 1 && rows <= kMaxRows, SHDR_E_SHAPE, "%s: a chunk holds 1 .. 32 scanlines, got %d", what, rows);
  SHDR_REQUIRE(n_chan >= 1 && n_chan <= kMaxChannels, SHDR_E_SHAPE, "%s: a chunk holds 1 .. 64 channels, got %d", what, n_chan);
  for (int c = 0; c < n_chan; ++c)
    SHDR_REQUIRE(chan_words[c] == 1 || chan_words[c] == 2, SHDR_E_SHAPE, "%s: channel %d has %d words (1: HALF, 2: FLOAT / UINT)", what, c,
                 chan_words[c]);
  const int64_t values = chunk_values(width, rows, chan_words, n_chan);
  SHDR_REQUIRE(values > 0 && n == 2 * values, SHDR_E_SHAPE,
               "%s: %lld bytes for a chunk of width %d, %d rows, %d channels (its shape holds %lld; at most 2^28)", what, (long long)n, width,
               rows, n_chan, (long long)(2 * values));
  const size_t sym = kSymPad;
  uint8_t* mem = static_cast<uint8_t*>(malloc(8 * sym * 2 + 4 * sym * 5 + 4 * 2 * kBitmapWords + 2 * (size_t)values + sym));
  SHDR_REQUIRE(mem, SHDR_E_SHAPE, "%s: out of memory", what);
  EncWork w;
  w.keys = reinterpret_cast<uint64_t*>(mem);
  w.code = w.keys + sym;
  w.freq = reinterpret_cast<uint32_t*>(w.code + sym);
  w.weight = w.freq + sym;
  w.made = w.weight + sym;
  w.parent = w.made + sym;                                       // 2 sym
  w.words = w.parent + 2 * sym;
  w.before = w.words + kBitmapWords;
  w.values = reinterpret_cast<uint16_t*>(w.before + kBitmapWords);
  w.lens = reinterpret_cast<uint8_t*>(w.values + values);
  const int64_t r = encode_host(raw, width, rows, chan_words, n_chan, dst, capacity, w);
  free(mem);
  SHDR_REQUIRE(r >= 0, SHDR_E_SHAPE, "%s: output buffer too small (%lld bytes; shdr_piz_encode_bound gives what always suffices)", what,
               (long long)capacity);
  *written = r;
  return SHDR_OK;
}

extern "C" int shdr_piz_encode_batch_sizes(const int64_t* chunk_off, const int32_t* geom, const int32_t* chan_words, int n_words, int n_chunks,
                                           int pad, int64_t* out_bytes, int64_t* workspace_bytes) {
  Plan p;
  if (int rc = make_plan("piz_encode_batch_sizes", chunk_off, geom, chan_words, n_words, n_chunks, pad, p)) return rc;
  if (out_bytes) *out_bytes = p.out_bytes;
  if (workspace_bytes) *workspace_bytes = p.ws_bytes;
  return SHDR_OK;
}

extern "C" int shdr_piz_encode_batch(const uint8_t* planar, const int64_t* chunk_off, const int64_t* chunk_off_dev, const int32_t* geom,
                                     const int32_t* geom_dev, const int32_t* chan_words, const int32_t* chan_words_dev, int n_words, int n_chunks,
                                     int pad, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, uint8_t* coded, void* workspace,
                                     int64_t workspace_bytes, int32_t* stats, void* stream, float* stage_ms) {
  const char* what = "piz_encode_batch";
  SHDR_REQUIRE(planar && chunk_off_dev && geom_dev && chan_words_dev && out && out_offsets && coded && workspace, SHDR_E_NULL,
               "%s: null pointer", what);
  Plan p;
  if (int rc = make_plan(what, chunk_off, geom, chan_words, n_words, n_chunks, pad, p)) return rc;
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(chunk_off_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out_offsets) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(geom_dev) & 3u) == 0 && (reinterpret_cast<uintptr_t>(chan_words_dev) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(planar) & 1u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3u) == 0 &&
                   shdr::aligned16(workspace),
               SHDR_E_ALIGN, "%s: chunk_off_dev and out_offsets must be 8-byte aligned, the shape tables 4-byte, planar 2-byte, the workspace 16-byte",
               what);
  SHDR_REQUIRE(out_capacity >= p.out_bytes, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_capacity,
               (long long)p.out_bytes);
  SHDR_REQUIRE(workspace_bytes >= p.ws_bytes, SHDR_E_SHAPE, "%s: the workspace holds %lld bytes, %lld are needed", what,
               (long long)workspace_bytes, (long long)p.ws_bytes);
  const Ws ws = carve(workspace, n_chunks, p.total);
  const Tables tb{chunk_off_dev, geom_dev, chan_words_dev, p.total, n_words};
  hipStream_t st = shdr::stream_of(stream);
  const dim3 grid((unsigned)n_chunks);
  shdr::StageTimer<SHDR_PIZ_ENC_STAGES> timer(stage_ms, st);
  if (hipMemsetAsync(ws.zero, 0, (size_t)ws.zero_bytes, st) != hipSuccess) return shdr::check_launch(what);
  timer.mark();
  hipLaunchKernelGGL(piz_enc_front_kernel, grid, dim3(kWide), 0, st, planar, tb, ws);
  timer.mark();
  hipLaunchKernelGGL(piz_enc_hist_kernel, grid, dim3(kWide), 0, st, tb, ws);
  timer.mark();
  hipLaunchKernelGGL(piz_enc_code_kernel, grid, dim3(kCodeThreads), 0, st, ws);
  timer.mark();
  hipLaunchKernelGGL(piz_enc_bits_kernel, grid, dim3(kWide), 0, st, tb, ws, pad, coded);
  timer.mark();
  hipLaunchKernelGGL(piz_enc_scan_kernel, dim3(1), dim3(1024), 0, st, ws.sizes, (int64_t)n_chunks, out_offsets);
  timer.mark();
  hipLaunchKernelGGL(piz_enc_final_kernel, grid, dim3(kCopyThreads), 0, st, planar, tb, ws, pad, out_offsets, out, out_capacity, stats);
  timer.mark();
  return shdr::check_launch(what);
}
