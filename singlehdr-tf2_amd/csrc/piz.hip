// OpenEXR PIZ chunks of a BATCH decoded on the device: the rules are those of piz.h, the very code of the host routine
// shdr_piz_decode_host, so the checks (and the per-chunk status codes) are the same on both sides.
//
// Two launches.  piz_decode_kernel, one 256-lane workgroup per chunk:
//   1. header: the fixed fields; the reverse LUT (every lane counts the set bits of 32 bitmap bytes, a scan over the lanes, every lane
//      writes its 256 values' entries); the code-length table unpacked by one lane (its tokens are variable-length); a counting sort of
//      the symbols by length across the lanes (each lane owns a column of the per-length counters: no atomics); the canonical
//      first / count / start arrays; the first-level table of 2^12 entries in LDS, filled entry by entry with the walk that also
//      answers longer codes (so the table and the walk cannot disagree).
//   2. self-synchronising decode: the nBits of the chunk are cut into subsequences of sub_bits; a PIZ token carries its run count with
//      it, so the only decoder state is the bit position.  Subsequence i starts speculatively at its border, and in every round takes
//      the end of subsequence i - 1 of the round before (two buffers) as its start, decoding again only when that moved.  Round r has
//      subsequences 0 .. r right, whatever the bytes are, so the loop ends (measured: 3 - 7 rounds on 512 x 512 files, up to 34 on 4K ones).
//      All rounds run inside the workgroup, between barriers: the host does not take part.
//   3. scan: an exclusive prefix sum of the subsequences' value counts and the "rightmost value that is no run" before each of them.
//   4. write: every subsequence is decoded once more from its true state into the u16 workspace; errors are judged only here, and the
//      first in stream order is the chunk's status.
// piz_wavelet_kernel, one workgroup per (chunk, channel word plane, strip of P columns), P the largest power of two <= min(width, rows)
// <= 32: aligned strips of P columns never touch each other at any level of the inverse wavelet (blocks are aligned to 2p <= P, and
// the left-over column of a level lies in the last, partial strip), so a strip runs all levels in LDS with a barrier between them,
// applies the LUT and writes the little-endian scanline layout into the chunk's slot.  A chunk with a status leaves its slot untouched.
// Deterministic, no atomics, no host wait, no allocation.
#include "shdr_internal.h"
#include "batch.h"
#include "piz.h"

namespace {

using namespace shdr_piz;

constexpr int kThreads = 256;
constexpr int kDefaultSubBits = 256;                            // measured: 256 / 1024 / 4096 / 16384 take 6.6 / 7.2 / 8.5 / 9.4 ms on 544 4K chunks
constexpr int kSymBlock = (kSymbols + kThreads - 1) / kThreads;  // symbols per lane of the counting sort: 257

// per-chunk workspace: what the two kernels hand over, then the tables
struct Meta {
  int32_t status;
  uint32_t max_value;
};
constexpr int64_t kMetaAt = 0;
constexpr int64_t kLutAt = 64;                                   // uint16 [65536]
constexpr int64_t kSortedAt = kLutAt + 2 * (int64_t)kLutSize;    // uint16 [65537 (+ pad)]
constexpr int64_t kLensAt = kSortedAt + 2 * 65600;               // uint8 [65537 (+ pad)]
constexpr int64_t kChunkWs = kLensAt + 65600;                    // a multiple of 16
static_assert(kChunkWs % 16 == 0, "per-chunk workspace keeps 16-byte alignment");
constexpr int kSubArrays = 7;                                    // uint32 each: end[2], used, count, last, offs, prev

struct Geom {                                 // int32 [4] per chunk
  int32_t width, rows, chan_first, n_chan;
};

// the first subsequence record of chunk c: chunk c has room for (8 bytes / sub_bits) + 1 of them
__device__ __host__ inline int64_t sub_base(int64_t src_lo, int64_t c, int sub_bits) { return 8 * src_lo / sub_bits + c; }

__global__ __launch_bounds__(kThreads) void piz_decode_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ src_off,
                                                              int64_t dst_bytes, const int64_t* __restrict__ dst_off,
                                                              const uint8_t* __restrict__ mode, const int32_t* __restrict__ geom,
                                                              const int32_t* __restrict__ chan_words, int n_words, uint8_t* __restrict__ dst,
                                                              uint8_t* __restrict__ ws, int64_t tmp_at, int64_t sub_at, int64_t total_subs,
                                                              int sub_bits, int32_t* __restrict__ status, int64_t* __restrict__ written,
                                                              int32_t* __restrict__ rounds_out) {
  __shared__ Canon canon;
  __shared__ uint32_t fast[1 << kFastBits];
  __shared__ uint16_t cnt[(kMaxLen + 1) * kThreads];
  __shared__ Head head;
  __shared__ int s_status;
  __shared__ uint32_t s_part[kThreads];
  __shared__ uint32_t s_last[kThreads];
  __shared__ uint64_t s_sum[kThreads];
  __shared__ int s_changed[2];

  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  const shdr::Span from = shdr::clamped_span(src_off, c, src_bytes, kMaxChunk), slot = shdr::clamped_span(dst_off, c, dst_bytes, kMaxChunk);
  const int64_t slo = from.lo, n = from.n, dlo = slot.lo, cap = slot.n;
  uint8_t* cws = ws + c * kChunkWs;
  Meta* meta = reinterpret_cast<Meta*>(cws + kMetaAt);
  uint16_t* lut = reinterpret_cast<uint16_t*>(cws + kLutAt);
  uint16_t* sorted = reinterpret_cast<uint16_t*>(cws + kSortedAt);
  uint8_t* lens = cws + kLensAt;
  const uint8_t* chunk = src + slo;
  const uint32_t m = mode ? mode[c] : 1u;

  // the shape, checked again (the host tables were validated before the launch; these are their device copies)
  Geom g{geom[4 * c], geom[4 * c + 1], geom[4 * c + 2], geom[4 * c + 3]};
  int64_t values = 0;
  if (g.chan_first >= 0 && g.n_chan >= 1 && (int64_t)g.chan_first + g.n_chan <= n_words)
    values = chunk_values(g.width, g.rows, chan_words + g.chan_first, g.n_chan);
  const bool shape_ok = values > 0 && 2 * values == cap && (dlo & 1) == 0;

  if (m != 1u || !shape_ok) {                                    // stored raw, or nothing to decode
    int st;
    int64_t wrote = 0;
    if (m == 0u && shape_ok) {
      if (n == cap) {
        for (int64_t i = t; i < n; i += kThreads) dst[dlo + i] = chunk[i];
        wrote = n;
        st = kOk;
      } else {
        st = kRawSize;
      }
    } else {
      st = m > 1u ? kMode : kRawSize;                            // a slot that is not the shape's size
    }
    if (t == 0) {
      meta->status = st ? st : -1;                               // -1: good, and nothing left for the wavelet kernel to do
      meta->max_value = 0;
      status[c] = st;
      written[c] = wrote;
      if (rounds_out)
        for (int i = 0; i < SHDR_PIZ_ROUND_STATS; ++i) rounds_out[c * SHDR_PIZ_ROUND_STATS + i] = 0;
    }
    return;
  }

  // ---- 1. header ------------------------------------------------------------------------------------------------------------
  if (t == 0) s_status = parse_head(chunk, n, head);
  for (int s = t; s < 65600; s += kThreads) lens[s] = 0;
  for (int i = t; i < (kMaxLen + 1) * kThreads; i += kThreads) cnt[i] = 0;
  __syncthreads();
  int st = s_status;
  if (st == kOk) {
    // reverse LUT: lane t owns the values 256 t .. 256 t + 255, bitmap bytes 32 t .. 32 t + 31
    uint32_t bits[8];
    uint32_t mine = 0;
    for (int w = 0; w < 8; ++w) {
      uint32_t v = 0;
      for (int k = 0; k < 4; ++k) {
        const uint32_t byte = 32u * t + 4u * w + k;
        if (byte >= head.bm_min && byte <= head.bm_max) v |= (uint32_t)chunk[head.bm_at + (byte - head.bm_min)] << (8 * k);
      }
      if (t == 0 && w == 0) v |= 1u;                             // value 0 is always present
      bits[w] = v;
      mine += __builtin_popcount(v);
    }
    s_part[t] = mine;
    __syncthreads();
    if (t == 0) {
      uint32_t run = 0;
      for (int i = 0; i < kThreads; ++i) {
        const uint32_t x = s_part[i];
        s_part[i] = run;
        run += x;
      }
      s_last[0] = run;                                           // the number of values present
    }
    __syncthreads();
    uint32_t k = s_part[t];
    const uint32_t present = s_last[0];
    for (int w = 0; w < 8; ++w)
      for (uint32_t v = bits[w]; v; v &= v - 1) lut[k++] = (uint16_t)(256u * t + 32u * w + (uint32_t)__builtin_ctz(v));
    for (uint32_t i = present + t; i < (uint32_t)kLutSize; i += kThreads) lut[i] = 0;
    // the code-length table: one lane
    if (t == 0) {
      s_status = unpack_lengths(chunk, head, lens);
      meta->max_value = present - 1;
    }
    __syncthreads();
    st = s_status;
  }
  if (st == kOk) {
    // counting sort by length: lane t owns the symbols kSymBlock t .. and column t of cnt
    const int s0 = t * kSymBlock, s1 = s0 + kSymBlock < kSymbols ? s0 + kSymBlock : kSymbols;
    for (int s = s0; s < s1; ++s) {
      const int l = lens[s];
      if (l) ++cnt[l * kThreads + t];
    }
    __syncthreads();
    if (t >= 1 && t <= kMaxLen) {                                // lane l: exclusive scan of the row of length l
      uint32_t run = 0;
      for (int i = 0; i < kThreads; ++i) {
        const uint32_t x = cnt[t * kThreads + i];
        cnt[t * kThreads + i] = (uint16_t)run;                   // the symbols before lane i's: at most 65535
        run += x;
      }
      canon.count[t] = run;
    }
    __syncthreads();
    if (t == 0) {
      s_status = make_canon(canon);
      canon.run_index = kNone;
    }
    __syncthreads();
    st = s_status;
    if (st == kOk) {
      for (int s = s0; s < s1; ++s) {
        const int l = lens[s];
        if (!l) continue;
        // (the largest symbol is the last of its length: the one whose count before it, 65536, a uint16 cannot hold)
        const uint32_t idx = s == kSymbols - 1 ? canon.start[l] + canon.count[l] - 1 : canon.start[l] + (uint32_t)cnt[l * kThreads + t]++;
        sorted[idx] = (uint16_t)s;
        if ((uint32_t)s == head.iM) canon.run_index = idx;       // one lane at most
      }
    }
    __syncthreads();
    if (st == kOk)
      for (uint32_t i = t; i < (1u << kFastBits); i += kThreads) fast[i] = fast_entry(canon, sorted, i);
    __syncthreads();
  }
  if (st != kOk) {
    if (t == 0) {
      meta->status = st;
      status[c] = st;
      written[c] = 0;
      if (rounds_out)
        for (int i = 0; i < SHDR_PIZ_ROUND_STATS; ++i) rounds_out[c * SHDR_PIZ_ROUND_STATS + i] = 0;
    }
    return;
  }

  // ---- 2. self-synchronising decode ---------------------------------------------------------------------------------------------
  const Code code{chunk + head.data_at, head.data_len, head.n_bits, &canon, fast, sorted};
  const uint64_t n_bits = head.n_bits;
  const int64_t n_sub = (int64_t)((n_bits + (uint64_t)sub_bits - 1) / (uint64_t)sub_bits);       // >= 1; fits the chunk's room
  uint32_t* sub = reinterpret_cast<uint32_t*>(ws + sub_at) + sub_base(slo, c, sub_bits);
  uint32_t* end0 = sub;
  uint32_t* end1 = sub + total_subs;
  uint32_t* used = sub + 2 * total_subs;
  uint32_t* count = sub + 3 * total_subs;
  uint32_t* last = sub + 4 * total_subs;
  uint32_t* offs = sub + 5 * total_subs;                         // the values before the subsequence (< 2^27: fits)
  uint32_t* prev = sub + 6 * total_subs;
  int rounds = 0;
  for (int64_t r = 0; r <= n_sub; ++r) {
    const uint32_t* rd = (r & 1) ? end1 : end0;
    uint32_t* wr = (r & 1) ? end0 : end1;
    if (t == 0) s_changed[(r + 1) & 1] = 0;
    int changed = 0;
    for (int64_t i = t; i < n_sub; i += kThreads) {
      const uint64_t border = (uint64_t)i * (uint64_t)sub_bits;
      uint64_t stop = border + (uint64_t)sub_bits;
      if (stop > n_bits) stop = n_bits;
      uint64_t start = i == 0 ? 0 : r == 0 ? border : rd[i - 1];
      if (r > 0 && (uint32_t)start == used[i]) {
        wr[i] = rd[i];
        continue;
      }
      uint32_t e, k, lv;
      span_scan(code, start, stop, e, k, lv);
      if (start >= stop) e = (uint32_t)start;                    // a token that ends beyond this subsequence's own border
      used[i] = (uint32_t)start;
      wr[i] = e;
      count[i] = k;
      last[i] = lv;
      ++changed;
    }
    if (changed) s_changed[r & 1] = 1;                           // (every writer stores the same 1)
    const bool stats = rounds_out && r + 1 < SHDR_PIZ_ROUND_STATS;   // measurement: the subsequences this round decoded
    if (stats) s_part[t] = (uint32_t)changed;
    __syncthreads();
    if (stats && t == 0) {                                       // (the next round's s_part is written behind the barrier below)
      uint32_t sum = 0;
      for (int i = 0; i < kThreads; ++i) sum += s_part[i];
      rounds_out[c * SHDR_PIZ_ROUND_STATS + 1 + r] = (int32_t)(sum > 0x7FFFFFFFu ? 0x7FFFFFFFu : sum);
    }
    rounds = (int)r + 1;
    if (!s_changed[r & 1]) break;
    __syncthreads();
  }
  // the ends of the last round written are in the buffer that the next round would read
  const uint32_t* fin = (rounds & 1) ? end1 : end0;
  if (rounds_out && t == 0)
    for (int i = rounds; i + 1 < SHDR_PIZ_ROUND_STATS; ++i) rounds_out[c * SHDR_PIZ_ROUND_STATS + 1 + i] = 0;

  // ---- 3. scan: contiguous blocks of subsequences per lane, the lanes' totals through LDS -----------------------------------------------
  const int64_t per = (n_sub + kThreads - 1) / kThreads;
  const int64_t b0 = t * per < n_sub ? t * per : n_sub, b1 = b0 + per < n_sub ? b0 + per : n_sub;
  {
    uint64_t sum = 0;
    uint32_t lv = kNone;
    for (int64_t i = b0; i < b1; ++i) {
      sum += count[i];
      if (last[i] != kNone) lv = last[i];
    }
    s_sum[t] = sum;
    s_last[t] = lv;
  }
  __syncthreads();
  if (t == 0) {
    uint64_t run = 0;
    uint32_t lv = kNone;
    for (int i = 0; i < kThreads; ++i) {
      const uint64_t x = s_sum[i];
      const uint32_t y = s_last[i];
      s_sum[i] = run;
      s_last[i] = lv;
      run += x;
      if (y != kNone) lv = y;
    }
    s_part[0] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)run;    // all values of the stream, saturated
  }
  __syncthreads();
  {
    uint64_t run = s_sum[t];
    uint32_t lv = s_last[t];
    for (int64_t i = b0; i < b1; ++i) {
      offs[i] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)run;
      prev[i] = lv;
      run += count[i];
      if (last[i] != kNone) lv = last[i];
    }
  }
  __syncthreads();

  // ---- 4. write: from true states; the first error in stream order is the status --------------------------------------------------------
  uint16_t* tmp = reinterpret_cast<uint16_t*>(ws + tmp_at + dlo);
  const uint64_t expected = (uint64_t)values;
  int64_t bad_at = n_sub;
  int bad = kOk;
  for (int64_t i = t; i < n_sub; i += kThreads) {
    uint64_t stop = ((uint64_t)i + 1) * (uint64_t)sub_bits;
    if (stop > n_bits) stop = n_bits;
    const uint64_t start = i == 0 ? 0 : fin[i - 1];
    uint64_t at = offs[i];                                       // saturated: beyond `expected` either way
    const int e = span_write(code, start, stop, tmp, at, expected, prev[i]);
    if (e != kOk && i < bad_at) {
      bad_at = i;
      bad = e;
    }
  }
  s_sum[t] = (uint64_t)bad_at;
  s_last[t] = (uint32_t)bad;
  __syncthreads();
  if (t == 0) {
    int64_t at = n_sub;
    int e = kOk;
    for (int i = 0; i < kThreads; ++i)
      if ((int64_t)s_sum[i] < at) {
        at = (int64_t)s_sum[i];
        e = (int)s_last[i];
      }
    if (e == kOk && (uint64_t)s_part[0] < expected) e = kTooFew;
    meta->status = e;
    status[c] = e;
    written[c] = e == kOk ? cap : 0;
    if (rounds_out) rounds_out[c * SHDR_PIZ_ROUND_STATS] = rounds;
  }
}

// one strip of one word plane: all levels in LDS, the LUT, the scanline layout
__global__ __launch_bounds__(kThreads) void piz_wavelet_kernel(const uint8_t* __restrict__ ws, int64_t tmp_at, int64_t dst_bytes,
                                                               const int64_t* __restrict__ dst_off, const int32_t* __restrict__ geom,
                                                               const int32_t* __restrict__ chan_words, int n_words, uint8_t* __restrict__ dst) {
  __shared__ uint16_t tile[kMaxRows][kMaxRows + 1];
  const int64_t c = blockIdx.x;
  const int t = threadIdx.x;
  const uint8_t* cws = ws + c * kChunkWs;
  const Meta* meta = reinterpret_cast<const Meta*>(cws + kMetaAt);
  if (meta->status != kOk) return;                               // refused, or stored raw: nothing to do
  const Geom g{geom[4 * c], geom[4 * c + 1], geom[4 * c + 2], geom[4 * c + 3]};
  if (g.chan_first < 0 || g.n_chan < 1 || (int64_t)g.chan_first + g.n_chan > n_words) return;   // (the decode kernel refused these)
  const int32_t* cw = chan_words + g.chan_first;
  const int nx = g.width, ny = g.rows;
  const int P = top_power(nx < ny ? nx : ny);
  const int x0 = (int)blockIdx.z * P;
  if (x0 >= nx) return;
  // which channel and word this plane is
  int plane = (int)blockIdx.y, ch = 0;
  int64_t value_at = 0, row_at = 0, row_words = 0;
  for (int k = 0; k < g.n_chan; ++k) row_words += (int64_t)nx * cw[k];
  for (; ch < g.n_chan && plane >= cw[ch]; ++ch) {
    plane -= cw[ch];
    value_at += (int64_t)nx * ny * cw[ch];
    row_at += (int64_t)nx * cw[ch];
  }
  if (ch >= g.n_chan) return;
  const int words = cw[ch], j = plane;
  const shdr::Span slot = shdr::clamped_span(dst_off, c, dst_bytes, kMaxChunk);
  const int64_t dlo = slot.lo, cap = slot.n;
  if (2 * row_words * ny != cap) return;
  const uint16_t* tmp = reinterpret_cast<const uint16_t*>(ws + tmp_at + dlo) + value_at;
  const uint16_t* lut = reinterpret_cast<const uint16_t*>(cws + kLutAt);
  const int w = nx - x0 < P ? nx - x0 : P;                       // columns of this strip
  for (int i = t; i < ny * w; i += kThreads) {
    const int y = i / w, x = i % w;
    tile[y][x] = tmp[((int64_t)y * nx + x0 + x) * words + j];
  }
  __syncthreads();
  const bool w14 = meta->max_value < 16384u;
  for (int p = P >> 1, p2 = P; p >= 1; p2 = p, p >>= 1) {
    const int bx = w >= p2 ? (w - p2) / p2 + 1 : 0, by = ny >= p2 ? (ny - p2) / p2 + 1 : 0;    // whole blocks
    const int xs = bx * p2, ys = by * p2;                        // where the loops stop
    const int colx = (w & p) ? 1 : 0, rowy = (ny & p) ? 1 : 0;
    const int items = by * (bx + colx) + rowy * bx;
    for (int i = t; i < items; i += kThreads) {
      if (i < by * (bx + colx)) {
        const int y = (i / (bx + colx)) * p2, k = i % (bx + colx);
        if (k < bx) {
          const int x = k * p2;
          if (w14) dec_quad<true>(tile[y][x], tile[y][x + p], tile[y + p][x], tile[y + p][x + p]);
          else dec_quad<false>(tile[y][x], tile[y][x + p], tile[y + p][x], tile[y + p][x + p]);
        } else {
          if (w14) dec<true>(tile[y][xs], tile[y + p][xs], tile[y][xs], tile[y + p][xs]);
          else dec<false>(tile[y][xs], tile[y + p][xs], tile[y][xs], tile[y + p][xs]);
        }
      } else {
        const int x = (i - by * (bx + colx)) * p2;
        if (w14) dec<true>(tile[ys][x], tile[ys][x + p], tile[ys][x], tile[ys][x + p]);
        else dec<false>(tile[ys][x], tile[ys][x + p], tile[ys][x], tile[ys][x + p]);
      }
    }
    __syncthreads();
  }
  uint16_t* out = reinterpret_cast<uint16_t*>(dst + dlo);        // 2-byte aligned: checked by the caller
  for (int i = t; i < ny * w; i += kThreads) {
    const int y = i / w, x = i % w;
    out[(int64_t)y * row_words + row_at + (int64_t)(x0 + x) * words + j] = lut[tile[y][x]];
  }
}

struct Plan {
  int64_t src_bytes, dst_bytes, ws_bytes, tmp_at, sub_at, total_subs;
  int max_strips, max_planes;
};

int make_plan(const char* what, const int64_t* src_off, const int64_t* dst_off, const int32_t* geom, const int32_t* chan_words, int n_words,
              int n_chunks, int sub_bits, int64_t src_total, int64_t dst_total, Plan& p) {
  SHDR_REQUIRE(src_off && dst_off && geom && chan_words, SHDR_E_NULL, "%s: null table", what);
  SHDR_REQUIRE(n_chunks > 0 && n_words > 0, SHDR_E_SHAPE, "%s: the numbers of chunks and channel words must be positive, got %d and %d", what,
               n_chunks, n_words);
  SHDR_REQUIRE(sub_bits >= kMinSubBits && sub_bits <= (1 << 20), SHDR_E_SHAPE, "%s: sub_bits must be %d .. 2^20, got %d", what, kMinSubBits,
               sub_bits);
  SHDR_REQUIRE(src_off[0] >= 0 && dst_off[0] >= 0, SHDR_E_SHAPE, "%s: an offset table starts below 0", what);
  p.max_strips = p.max_planes = 1;
  for (int c = 0; c < n_chunks; ++c) {
    const int64_t n = src_off[c + 1] - src_off[c], cap = dst_off[c + 1] - dst_off[c];
    SHDR_REQUIRE(n >= 0 && n <= kMaxChunk, SHDR_E_SHAPE, "%s: chunk %d has %lld stored bytes (0 .. 2^28 are supported)", what, c, (long long)n);
    const Geom g{geom[4 * c], geom[4 * c + 1], geom[4 * c + 2], geom[4 * c + 3]};
    SHDR_REQUIRE(g.chan_first >= 0 && g.n_chan >= 1 && (int64_t)g.chan_first + g.n_chan <= n_words, SHDR_E_SHAPE,
                 "%s: chunk %d: channels %d .. %d + %d lie outside the table of %d", what, c, g.chan_first, g.chan_first, g.n_chan, n_words);
    const int64_t values = chunk_values(g.width, g.rows, chan_words + g.chan_first, g.n_chan);
    SHDR_REQUIRE(values > 0, SHDR_E_SHAPE,
                 "%s: chunk %d: width %d, rows %d, %d channels (1 .. 32 rows, 1 .. 64 channels of 1 or 2 words, at most 2^28 bytes)", what, c,
                 g.width, g.rows, g.n_chan);
    SHDR_REQUIRE(cap == 2 * values, SHDR_E_SHAPE, "%s: chunk %d: its slot has %lld bytes, its shape holds %lld", what, c, (long long)cap,
                 (long long)(2 * values));
    SHDR_REQUIRE((dst_off[c] & 1) == 0, SHDR_E_ALIGN, "%s: chunk %d: its slot starts at an odd byte", what, c);
    const int P = top_power(g.width < g.rows ? g.width : g.rows);
    const int strips = (g.width + P - 1) / P;
    int planes = 0;
    for (int k = 0; k < g.n_chan; ++k) planes += chan_words[g.chan_first + k];
    if (strips > p.max_strips) p.max_strips = strips;
    if (planes > p.max_planes) p.max_planes = planes;
  }
  SHDR_REQUIRE(p.max_strips <= 65535, SHDR_E_SHAPE, "%s: a chunk is too wide", what);
  p.src_bytes = src_off[n_chunks];
  p.dst_bytes = dst_off[n_chunks];
  SHDR_REQUIRE(src_total < 0 || p.src_bytes <= src_total, SHDR_E_SHAPE, "%s: src_off ends at %lld, the buffer holds %lld bytes", what,
               (long long)p.src_bytes, (long long)src_total);
  SHDR_REQUIRE(dst_total < 0 || p.dst_bytes <= dst_total, SHDR_E_SHAPE, "%s: dst_off ends at %lld, the buffer holds %lld bytes", what,
               (long long)p.dst_bytes, (long long)dst_total);
  p.tmp_at = (int64_t)n_chunks * kChunkWs;
  p.sub_at = (p.tmp_at + p.dst_bytes + 15) & ~(int64_t)15;
  p.total_subs = sub_base(p.src_bytes, n_chunks, sub_bits) + 1;
  p.ws_bytes = p.sub_at + 4 * kSubArrays * p.total_subs;
  return SHDR_OK;
}

}  // namespace

extern "C" int64_t shdr_piz_decode_host(const uint8_t* src, int64_t n, int width, int rows, const int32_t* chan_words, int n_chan,
                                        uint8_t* dst, int64_t capacity, int* status) {
  const int64_t values = chunk_values(width, rows, chan_words, n_chan);
  if (!status || n < 0 || n > kMaxChunk || (!src && n) || values <= 0 || capacity != 2 * values || !dst) {
    shdr::set_error("piz_decode_host: bad arguments (null pointer, a size beyond 2^28 bytes, a shape out of range, or a capacity that is "
                    "not the shape's 2 * width * rows * words)");
    return -1;
  }
  uint8_t* mem = static_cast<uint8_t*>(malloc(65600 + 2 * 65600 + 4 * (1 << kFastBits) + 2 * kLutSize + 2 * (size_t)values));
  if (!mem) {
    shdr::set_error("piz_decode_host: out of memory");
    return -1;
  }
  HostWork w;
  w.fast = reinterpret_cast<uint32_t*>(mem);
  w.sorted = reinterpret_cast<uint16_t*>(mem + 4 * (1 << kFastBits));
  w.lut = w.sorted + 65600;
  w.values = w.lut + kLutSize;
  w.lens = reinterpret_cast<uint8_t*>(w.values + values);
  *status = decode_host(src, n, width, rows, chan_words, n_chan, dst, w);
  free(mem);
  return *status == kOk ? capacity : 0;
}

extern "C" int shdr_piz_batch_sizes(const int64_t* src_off, const int64_t* dst_off, const int32_t* geom, const int32_t* chan_words, int n_words,
                                    int n_chunks, int sub_bits, int64_t* src_bytes, int64_t* dst_bytes, int64_t* workspace_bytes) {
  Plan p;
  if (int rc = make_plan("piz_batch_sizes", src_off, dst_off, geom, chan_words, n_words, n_chunks, sub_bits > 0 ? sub_bits : kDefaultSubBits, -1,
                         -1, p))
    return rc;
  if (src_bytes) *src_bytes = p.src_bytes;
  if (dst_bytes) *dst_bytes = p.dst_bytes;
  if (workspace_bytes) *workspace_bytes = p.ws_bytes;
  return SHDR_OK;
}

extern "C" int shdr_piz_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* src_off_dev, uint8_t* dst,
                              int64_t dst_bytes, const int64_t* dst_off, const int64_t* dst_off_dev, const uint8_t* mode, const int32_t* geom,
                              const int32_t* geom_dev, const int32_t* chan_words, const int32_t* chan_words_dev, int n_words, int n_chunks,
                              int sub_bits, void* workspace, int64_t workspace_bytes, int32_t* status, int64_t* written, int32_t* rounds,
                              void* stream, float* stage_ms) {
  const char* what = "piz_batch";
  SHDR_REQUIRE(src_off_dev && dst_off_dev && geom_dev && chan_words_dev && status && written && workspace, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(src_bytes >= 0 && dst_bytes >= 0 && (src || !src_bytes) && (dst || !dst_bytes), SHDR_E_NULL, "%s: null buffer", what);
  if (sub_bits <= 0) sub_bits = kDefaultSubBits;
  Plan p;
  if (int rc = make_plan(what, src_off, dst_off, geom, chan_words, n_words, n_chunks, sub_bits, src_bytes, dst_bytes, p)) return rc;
  SHDR_REQUIRE(workspace_bytes >= p.ws_bytes, SHDR_E_SHAPE, "%s: the workspace holds %lld bytes, %lld are needed", what,
               (long long)workspace_bytes, (long long)p.ws_bytes);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(src_off_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(dst_off_dev) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(written) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(geom_dev) & 3u) == 0 && (reinterpret_cast<uintptr_t>(chan_words_dev) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && (reinterpret_cast<uintptr_t>(dst) & 1u) == 0,
               SHDR_E_ALIGN, "%s: the offset tables and `written` must be 8-byte aligned, `status` and the shape tables 4-byte, the workspace 16-byte, dst 2-byte", what);
  hipStream_t st = shdr::stream_of(stream);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  shdr::StageTimer<SHDR_PIZ_STAGES> timer(stage_ms, st);
  hipLaunchKernelGGL(piz_decode_kernel, dim3((unsigned)n_chunks), dim3(kThreads), 0, st, src, p.src_bytes, src_off_dev, p.dst_bytes, dst_off_dev,
                     mode, geom_dev, chan_words_dev, n_words, dst, ws, p.tmp_at, p.sub_at, p.total_subs, sub_bits, status, written, rounds);
  timer.mark();
  hipLaunchKernelGGL(piz_wavelet_kernel, dim3((unsigned)n_chunks, (unsigned)p.max_planes, (unsigned)p.max_strips), dim3(kThreads), 0, st, ws,
                     p.tmp_at, p.dst_bytes, dst_off_dev, geom_dev, chan_words_dev, n_words, dst);
  timer.mark();
  return shdr::check_launch(what);
}
