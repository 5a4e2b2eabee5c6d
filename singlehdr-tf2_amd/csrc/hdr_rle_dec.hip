// Radiance .hdr scanline reader on the device: what shdr_rgbe_rle_decode (csrc/api.cpp) accepts, refuses and writes, for a BATCH of
// files of different shapes in one call.  The rules are csrc/hdr_rle_dec.h, the code of the host twin shdr_rgbe_rle_decode_status.
//
// A Radiance file has no index: where line y + 1 starts is known only after line y has been walked, and whether a line is coded or
// flat is decided by the four bytes found there.  But whether an offset p holds the line marker (p is a CANDIDATE) and what a parse of
// one coded line from p gives are properties of the bytes alone.  The line starts of a file are the orbit of offset 0 under
//     at a candidate: jump to the end of its parse (or stop with its failure);  elsewhere: step 4 W (or stop: truncated flat line)
// cut after H lines.  So every candidate is parsed at once, and the orbit is followed over the parsed candidates afterwards.
//
// A NODE is a candidate together with the flat lines that follow its coded line up to the next candidate; node 0 of a file is virtual
// (no coded line, "ends" at offset 0).  Candidates are kept in offset order, so a node's successor has a larger index.
//
// Stages (stream-ordered, no global atomics, no host wait, no allocation; the same input gives the same bytes):
//   1  mark      dec_setup_kernel (tables), dec_count_kernel (markers per 16 KiB chunk), dec_compact_kernel (candidates in offset order:
//                a block's base is the sum of the counts of the chunks in front of it).  A file with more than 2 H + 64 candidates is
//                SHDR_RGBE_DEC_FALLBACK: nothing further is done for it.  The encoder's output has exactly H.
//   2  parse     dec_parse_kernel, one wave per candidate: the packet chain is walked through a 1 KiB LDS window of the file that the wave
//                refills with 16-byte loads (a line may be padded with zero counts without limit, so it is staged in pieces; every packet
//                consumes a byte, so the walk ends).  Then the wave resolves its node's successor: flat steps from its end, merged against
//                the sorted candidate list.
//   3  rank      dec_rank_kernel, one workgroup per file: pointer doubling from node 0.  Round k holds jump[i] = next^(2^k)(i) and the lines
//                that jump covers; the nodes reached so far (distance < 2^k) mark their jump targets and hand them their row, then every
//                node doubles its jump.  ceil(log2(nodes)) rounds instead of a chain of H dependent loads.  The one node of the orbit
//                with a failure in a row < H decides status, line and stop; each row < H of the orbit gets a descriptor.
//   4  expand    dec_expand_kernel, one workgroup per row of the batch, wave c expands component c: the interleaved pixels of an x-tile of
//                2048 are assembled in LDS and stored as whole dwords; flat rows are a copy.
#include "shdr_internal.h"
#include "batch.h"
#include "hdr_rle_dec.h"

namespace {

using namespace shdr_rle_dec;

static_assert(kOk == SHDR_RGBE_DEC_OK && kTruncated == SHDR_RGBE_DEC_TRUNCATED && kCorruptRun == SHDR_RGBE_DEC_CORRUPT_RUN &&
                  kCorruptLiteral == SHDR_RGBE_DEC_CORRUPT_LITERAL && kTruncatedFlat == SHDR_RGBE_DEC_TRUNCATED_FLAT &&
                  kFallback == SHDR_RGBE_DEC_FALLBACK,
              "csrc/hdr_rle_dec.h and include/shdr.h list the same status codes");

constexpr int kChunk = 16384;                  // bytes per block of the marker passes
constexpr int kChunkPerThread = kChunk / 256;
constexpr int kWindow = 1024;                  // bytes of a wave's LDS window
constexpr int kTile = 2048;                    // pixels of an x-tile of the expander
constexpr int kMaxWidth = 1 << 28;             // 4 * W fits an int32 with room
constexpr int kMaxFiles = 65535;               // a grid dimension
constexpr int kNone = -1;
constexpr int kSat = 1 << 30;                  // line counts saturate here

__host__ __device__ inline int64_t cap_of(int h, int w) { return rle_width(w) ? 2 * (int64_t)h + 64 : 0; }
__host__ __device__ inline int64_t chunks_of(int64_t size, int w) { return rle_width(w) ? (size + kChunk - 1) / kChunk : 0; }

struct DecWorkspace {                          // carved out of the caller's workspace, every part 16-byte aligned
  int64_t* rowstart;                           // [N + 1] first row of file n among all rows
  int64_t* nodeoff;                            // [N + 1] first node of file n
  int64_t* chunkoff;                           // [N + 1] first chunk of file n
  int32_t* ncand;                              // [N]     candidates found (may exceed the cap)
  int32_t* chunkcnt;                           // [chunks]
  int32_t* n_pos;                              // per node: offset of the marker in the file (node 0: 0)
  int32_t* n_end;                              //           first byte after the coded line
  int32_t* n_fail;                             //           0, or the failure this node ends the orbit with ...
  int32_t* n_rel;                              //           ... in this line counted from the node's first ...
  int32_t* n_stop;                             //           ... at this offset
  int32_t* n_flat;                             //           flat lines that follow the coded line
  int32_t* n_mark;                             //           round in which the orbit reached the node, -1 if it has not
  int32_t* n_row;                              //           its first row
  int32_t* n_next[2];                          //           jump pointers, two buffers
  int32_t* n_len[2];                           //           lines the jump covers
  int32_t* n_comp;                             //  [nodes][4] first count byte of every component
  int32_t* rowdesc;                            //  [R][2] {offset of the line in its file or -1: nothing to write, node or -1: flat}
  int64_t bytes;
};
inline DecWorkspace carve(void* ws, int64_t n, int64_t rows, int64_t nodes, int64_t chunks) {
  DecWorkspace w;
  shdr::Carver cut(ws);
  auto i32 = [&](int64_t count) { return cut.take<int32_t>(count); };
  w.rowstart = cut.take<int64_t>(n + 1);
  w.nodeoff = cut.take<int64_t>(n + 1);
  w.chunkoff = cut.take<int64_t>(n + 1);
  w.ncand = i32(n);
  w.chunkcnt = i32(chunks);
  w.n_pos = i32(nodes); w.n_end = i32(nodes); w.n_fail = i32(nodes); w.n_rel = i32(nodes); w.n_stop = i32(nodes);
  w.n_flat = i32(nodes); w.n_mark = i32(nodes); w.n_row = i32(nodes);
  w.n_next[0] = i32(nodes); w.n_next[1] = i32(nodes); w.n_len[0] = i32(nodes); w.n_len[1] = i32(nodes);
  w.n_comp = i32(4 * nodes);
  w.rowdesc = i32(2 * rows);
  w.bytes = cut.bytes();
  return w;
}

constexpr int64_t kMaxFileBytes = 0x7fffffff;  // the cap of a file's clamped_span: offsets inside a file are int32

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void dec_setup_kernel(const int32_t* __restrict__ shapes, const int64_t* __restrict__ src_off, int64_t src_bytes, int n,
                                 int64_t* __restrict__ rowstart, int64_t* __restrict__ nodeoff, int64_t* __restrict__ chunkoff,
                                 int32_t* __restrict__ ncand, int64_t* __restrict__ out_off) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t r = 0, nd = 0, ch = 0, o = 0;
  for (int i = 0; i < n; ++i) {
    const int h = shapes[2 * i], w = shapes[2 * i + 1];
    rowstart[i] = r; nodeoff[i] = nd; chunkoff[i] = ch; out_off[i] = o;
    ncand[i] = 0;
    r += h;
    nd += cap_of(h, w) + 1;
    ch += chunks_of(shdr::clamped_span(src_off, i, src_bytes, kMaxFileBytes).n, w);
    o += 4 * (int64_t)h * w;
  }
  rowstart[n] = r; nodeoff[n] = nd; chunkoff[n] = ch; out_off[n] = o;
}

// markers among the kChunkPerThread offsets from p0 on (thread-private, in offset order); FN(offset) for each
template <class FN>
__device__ __forceinline__ int scan_markers(const uint8_t* __restrict__ data, int64_t size, int64_t p0, int w, FN&& fn) {
  int count = 0;
  int64_t p1 = p0 + kChunkPerThread;
  if (p1 > size - 3) p1 = size - 3;                                       // a marker needs four bytes
  for (int64_t p = p0; p < p1; ++p) {
    if (data[p] != 2 || data[p + 1] != 2) continue;
    if (marker_bytes(2, 2, data[p + 2], data[p + 3], w)) {
      fn(p, count);
      ++count;
    }
  }
  return count;
}

__device__ __forceinline__ int block_sum_256(int v, int* part) {          // every thread of a 256-thread block calls it
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(256) void dec_count_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ src_off,
                                                        const int32_t* __restrict__ shapes, const int64_t* __restrict__ chunkoff,
                                                        int32_t* __restrict__ chunkcnt) {
  __shared__ int part[4];
  const int f = blockIdx.y;
  const int64_t chunk = blockIdx.x;
  if (chunk >= chunkoff[f + 1] - chunkoff[f]) return;
  const shdr::Span fs = shdr::clamped_span(src_off, f, src_bytes, kMaxFileBytes);
  const int w = shapes[2 * f + 1];
  const int c = scan_markers(src + fs.lo, fs.n, chunk * kChunk + (int64_t)threadIdx.x * kChunkPerThread, w, [](int64_t, int) {});
  const int total = block_sum_256(c, part);
  if (threadIdx.x == 0) chunkcnt[chunkoff[f] + chunk] = total;
}

__global__ __launch_bounds__(256) void dec_compact_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ src_off,
                                                          const int32_t* __restrict__ shapes, const int64_t* __restrict__ chunkoff,
                                                          const int32_t* __restrict__ chunkcnt, const int64_t* __restrict__ nodeoff,
                                                          int32_t* __restrict__ ncand, int32_t* __restrict__ n_pos) {
  __shared__ int part[4];
  __shared__ int wave_base[4];
  const int f = blockIdx.y;
  const int64_t chunk = blockIdx.x, nch = chunkoff[f + 1] - chunkoff[f];
  if (chunk >= nch) return;
  const shdr::Span fs = shdr::clamped_span(src_off, f, src_bytes, kMaxFileBytes);
  const int h = shapes[2 * f], w = shapes[2 * f + 1];
  const int64_t cap = cap_of(h, w);
  const int32_t* cnt = chunkcnt + chunkoff[f];
  int64_t before = 0, all = 0;                                            // candidates in the chunks in front, and in the file
  for (int64_t i = threadIdx.x; i < nch; i += 256) {
    const int v = cnt[i];
    all += v;
    if (i < chunk) before += v;
  }
  // (two int sums: a file has fewer than 2^31 bytes, so fewer candidates)
  const int base = block_sum_256((int)before, part);
  const int total = block_sum_256((int)all, part);
  if (chunk == 0 && threadIdx.x == 0) ncand[f] = total;
  if (total > cap) return;                                                // FALLBACK: the list is not needed
  const uint8_t* data = src + fs.lo;
  const int64_t p0 = chunk * kChunk + (int64_t)threadIdx.x * kChunkPerThread;
  const int mine = scan_markers(data, fs.n, p0, w, [](int64_t, int) {});
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = shdr::wave_scan(mine);                                 // (not block_scan: wave_base is read once, no barrier behind it)
  if (lane == 63) wave_base[wave] = incl;
  __syncthreads();
  int at = base + incl - mine;
  for (int k = 0; k < wave; ++k) at += wave_base[k];
  int32_t* list = n_pos + nodeoff[f] + 1;                                 // node 0 is the virtual one
  if (mine) scan_markers(data, fs.n, p0, w, [&](int64_t p, int k) {
    if (at + k < cap) list[at + k] = (int32_t)p;
  });
}

// A wave's view of its file through kWindow bytes of LDS.  p is the same in every lane.  Bytes outside the buffer read as 0; bytes of a
// neighbouring file may be staged, and no rule looks at them: every use is checked against the file's size first.
struct WaveWindow {
  const uint8_t* src;
  int64_t src_bytes, fbase, lo;
  uint8_t* win;
  int lane;
  __device__ WaveWindow(const uint8_t* s, int64_t sb, int64_t fb, uint8_t* w, int l)
      : src(s), src_bytes(sb), fbase(fb), lo(-((int64_t)1 << 60)), win(w), lane(l) {}
  __device__ void stage(int64_t p) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(src) + (uintptr_t)(fbase + p);
    const int64_t g0 = fbase + p - (int64_t)(addr & 15u);                 // index in src of the aligned 16 bytes that hold p
    lo = g0 - fbase;
    const int64_t gl = g0 + 16 * lane;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (gl >= 0 && gl + 16 <= src_bytes) {
      v = *reinterpret_cast<const uint4*>(src + gl);
    } else {
      uint32_t t[4] = {0u, 0u, 0u, 0u};
      for (int j = 0; j < 16; ++j)
        if (gl + j >= 0 && gl + j < src_bytes) t[j >> 2] |= (uint32_t)src[gl + j] << (8 * (j & 3));
      v = make_uint4(t[0], t[1], t[2], t[3]);
    }
    wave_sync();                                                          // the reads of the old window are done
    reinterpret_cast<uint4*>(win)[lane] = v;
    wave_sync();
  }
  __device__ int operator()(int64_t p) {
    if (p < lo || p >= lo + kWindow) stage(p);
    return win[p - lo];
  }
};

// One wave per node.  Parse, then the successor: from the end of the coded line, flat steps until a candidate is hit, the file is left
// or H lines are counted; `list` is sorted, so the walk is a merge.
__global__ __launch_bounds__(64) void dec_parse_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ src_off,
                                                       const int32_t* __restrict__ shapes, int n_files, const int64_t* __restrict__ nodeoff,
                                                       const int32_t* __restrict__ ncand, const int32_t* __restrict__ n_pos,
                                                       int32_t* __restrict__ n_end, int32_t* __restrict__ n_fail, int32_t* __restrict__ n_rel,
                                                       int32_t* __restrict__ n_stop, int32_t* __restrict__ n_flat, int32_t* __restrict__ n_next,
                                                       int32_t* __restrict__ n_len, int32_t* __restrict__ n_comp) {
  __shared__ uint4 window[kWindow / 16];
  const int64_t node = blockIdx.x;
  const int f = (int)shdr::last_le(nodeoff, n_files, node);
  const int k = (int)(node - nodeoff[f]);
  const int h = shapes[2 * f], w = shapes[2 * f + 1];
  const int64_t cap = cap_of(h, w);
  const int m = ncand[f];
  if (m > cap || k > m) return;                                           // FALLBACK, or a slot no candidate fills
  const shdr::Span fs = shdr::clamped_span(src_off, f, src_bytes, kMaxFileBytes);
  const int lane = threadIdx.x;
  const int32_t* list = n_pos + nodeoff[f] + 1;
  int own = 0, fail = 0, rel = 0;
  int64_t e = 0, stop = 0;
  if (k > 0) {
    own = 1;
    WaveWindow read(src, src_bytes, fs.lo, reinterpret_cast<uint8_t*>(window), lane);
    Line l;
    parse_line(read, fs.n, list[k - 1], w, &l);
    if (lane == 0) *reinterpret_cast<int4*>(n_comp + 4 * node) = make_int4((int)l.comp[0], (int)l.comp[1], (int)l.comp[2], (int)l.comp[3]);
    if (l.status != kOk) {
      fail = l.status; stop = l.stop;
    }
    e = l.end;
  }
  int flat = 0, next = kNone;
  const int64_t coded_end = e;                                            // -1 behind a failed parse
  if (!fail) {
    const int64_t step = 4 * (int64_t)w;
    int idx = k;                                                          // candidates in front of list[k] start before e
    while (own + flat < h) {
      while (idx < m && list[idx] < e) ++idx;
      if (idx < m && list[idx] == e) {
        next = idx + 1;
        break;
      }
      if (fs.n - e < step) {
        fail = kTruncatedFlat; rel = own + flat; stop = e;
        break;
      }
      int64_t steps = (fs.n - e) / step;                               // whole flat lines left, at least one
      if (idx < m) {
        const int64_t want = (list[idx] - e + step - 1) / step;           // as many as reach the next candidate
        if (want < steps) steps = want;
      }
      if (steps > h - own - flat) steps = h - own - flat;
      e += steps * step;
      flat += (int)steps;
    }
  }
  if (lane == 0) {
    n_end[node] = (int32_t)coded_end;
    n_fail[node] = fail;
    n_rel[node] = rel;
    n_stop[node] = (int32_t)stop;
    n_flat[node] = flat;
    n_next[node] = next;
    n_len[node] = own + flat;
  }
}

// One workgroup per file: rows by pointer doubling, the file's report, the row descriptors.
__global__ __launch_bounds__(1024) void dec_rank_kernel(const int32_t* __restrict__ shapes, const int64_t* __restrict__ rowstart,
                                                        const int64_t* __restrict__ nodeoff, const int32_t* __restrict__ ncand,
                                                        const int32_t* __restrict__ n_pos, const int32_t* __restrict__ n_end,
                                                        const int32_t* __restrict__ n_fail, const int32_t* __restrict__ n_rel,
                                                        const int32_t* __restrict__ n_stop, const int32_t* __restrict__ n_flat,
                                                        int32_t* __restrict__ n_mark, int32_t* __restrict__ n_row, int32_t* next0,
                                                        int32_t* next1, int32_t* len0, int32_t* len1, int32_t* __restrict__ rowdesc,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ line,
                                                        int64_t* __restrict__ consumed) {
  __shared__ int s_status, s_line;
  __shared__ long long s_consumed;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int h = shapes[2 * f], w = shapes[2 * f + 1];
  const int64_t nb = nodeoff[f];
  const int m = ncand[f];
  int2* desc = reinterpret_cast<int2*>(rowdesc) + rowstart[f];
  for (int y = tid; y < h; y += 1024) desc[y] = make_int2(-1, -1);
  if (m > cap_of(h, w)) {
    if (tid == 0) {
      status[f] = kFallback; line[f] = -1; consumed[f] = -1;
    }
    return;
  }
  const int nodes = m + 1;
  n_mark += nb; n_row += nb; next0 += nb; next1 += nb; len0 += nb; len1 += nb;
  for (int i = tid; i < nodes; i += 1024) {
    n_mark[i] = i == 0 ? 0 : -1;
    n_row[i] = 0;
  }
  if (tid == 0) {
    s_status = kOk; s_line = -1; s_consumed = -1;
  }
  __syncthreads();
  int32_t *nx = next0, *ln = len0, *nx2 = next1, *ln2 = len1;
  int round = 1;
  for (int span = 1; span < nodes; span <<= 1, ++round) {
    for (int i = tid; i < nodes; i += 1024) {
      const int j = nx[i];
      const int mk = n_mark[i];
      if (j != kNone && mk >= 0 && mk < round) {                          // reached in an earlier round: its row is final
        const int64_t r = (int64_t)n_row[i] + ln[i];
        if (r < h) {                                                      // (one marked source per target: the orbit is a path)
          n_row[j] = (int)r;
          n_mark[j] = round;
        }
      }
      int j2 = kNone, l2 = ln[i];
      if (j != kNone) {
        j2 = nx[j];
        const int64_t t = (int64_t)l2 + ln[j];
        l2 = t > kSat ? kSat : (int)t;
      }
      nx2[i] = j2;
      ln2[i] = l2;
    }
    __syncthreads();
    int32_t* t = nx; nx = nx2; nx2 = t;
    t = ln; ln = ln2; ln2 = t;
  }
  n_pos += nb; n_end += nb; n_fail += nb; n_rel += nb; n_stop += nb; n_flat += nb;
  const int64_t step = 4 * (int64_t)w;
  for (int i = tid; i < nodes; i += 1024) {
    if (n_mark[i] < 0) continue;
    const int row = n_row[i], own = i > 0 ? 1 : 0, flat = n_flat[i], fail = n_fail[i];
    if (row >= h) continue;
    if (fail && (int64_t)row + n_rel[i] < h) {                            // the orbit ends here, inside the image
      s_status = fail; s_line = row + n_rel[i]; s_consumed = n_stop[i];
    }
    if (own && !(fail && n_rel[i] == 0)) desc[row] = make_int2(n_pos[i], i);
    const int64_t e = n_end[i];
    for (int k = 0; k < flat && (int64_t)row + own + k < h; ++k) desc[row + own + k] = make_int2((int)(e + k * step), -1);
    const int64_t last = (int64_t)h - 1 - row;                            // line h - 1 counted from this node's first
    if ((!fail || (int64_t)row + n_rel[i] >= h) && last < own + flat) s_consumed = e + (last - own + 1) * step;
  }
  __syncthreads();
  if (tid == 0) {
    status[f] = s_status; line[f] = s_line; consumed[f] = s_consumed;
  }
}

// One workgroup per row of the batch.  A coded row: wave c walks the packets of component c (its first count byte is the parser's) and
// the lanes write the bytes of a packet into the tile; a packet that crosses the tile's end is met again in the next tile.
__global__ __launch_bounds__(256) void dec_expand_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ src_off,
                                                         const int32_t* __restrict__ shapes, int n_files, const int64_t* __restrict__ rowstart,
                                                         const int64_t* __restrict__ nodeoff, const int32_t* __restrict__ n_comp,
                                                         const int32_t* __restrict__ rowdesc, const int64_t* __restrict__ out_off,
                                                         uint8_t* __restrict__ out, int64_t out_bytes) {
  __shared__ uint32_t tile[kTile];
  __shared__ uint4 window[4][kWindow / 16];
  const int64_t grow = blockIdx.x;
  const int f = (int)shdr::last_le(rowstart, n_files, grow);
  const int w = shapes[2 * f + 1];
  const int64_t row = grow - rowstart[f];
  const int2 d = reinterpret_cast<const int2*>(rowdesc)[grow];
  if (d.x < 0) return;                                                    // a refused or FALLBACK file, or a row behind a failure
  const int64_t at = out_off[f] + row * 4 * (int64_t)w;
  if (at < 0 || at + 4 * (int64_t)w > out_bytes) return;                  // never with the tables the host checked
  uint32_t* dst = reinterpret_cast<uint32_t*>(out + at);
  const shdr::Span fs = shdr::clamped_span(src_off, f, src_bytes, kMaxFileBytes);
  const uint8_t* data = src + fs.lo;
  if (d.y < 0) {                                                          // flat: a copy, the source at any alignment
    const int64_t p = d.x;
    if (p + 4 * (int64_t)w > fs.n) return;
    for (int x = threadIdx.x; x < w; x += 256) {
      const uint8_t* q = data + p + 4 * (int64_t)x;
      dst[x] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
    }
    return;
  }
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  WaveWindow read(src, src_bytes, fs.lo, reinterpret_cast<uint8_t*>(window[c]), lane);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(tile);
  int64_t pos = n_comp[4 * (nodeoff[f] + d.y) + c];
  int x = 0;
  for (int t0 = 0; t0 < w; t0 += kTile) {
    const int t1 = t0 + kTile < w ? t0 + kTile : w;
    while (x < t1) {
      int len = 0;
      bool run = false;
      int64_t next = pos;
      if (pos < 0 || pos >= fs.n || packet_step(read(pos), pos, fs.n, x, w, &len, &run, &next) != kOk) {
        x = w;                                                            // (the parser accepted this line: not reached)
        break;
      }
      const int lo = x > t0 ? x : t0, hi = x + len < t1 ? x + len : t1;
      if (run) {
        const int v = read(pos + 1);
        for (int i = lo + lane; i < hi; i += 64) bytes[4 * (i - t0) + c] = (uint8_t)v;
      } else {
        for (int i = lo + lane; i < hi; i += 64) bytes[4 * (i - t0) + c] = data[pos + 1 + (i - x)];
      }
      if (x + len > t1) break;                                            // the rest of this packet belongs to the next tile
      x += len;
      pos = next;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < t1 - t0; i += 256) dst[t0 + i] = tile[i];
    __syncthreads();
  }
}

struct Plan {
  int64_t rows, nodes, chunks, max_chunks, out_bytes;
};

// the tables as the ABI takes them: validated on the host, totals returned
int make_plan(const char* what, const int32_t* shapes, const int64_t* src_off, int n, int64_t src_bytes, Plan* p) {
  SHDR_REQUIRE(shapes && src_off, SHDR_E_NULL, "%s: null shape or offset table", what);
  SHDR_REQUIRE(n > 0 && n <= kMaxFiles, SHDR_E_SHAPE, "%s: the number of files must be 1 .. %d, got %d", what, kMaxFiles, n);
  *p = Plan{0, 0, 0, 0, 0};
  SHDR_REQUIRE(src_off[0] >= 0, SHDR_E_SHAPE, "%s: src_off[0] is negative", what);
  for (int i = 0; i < n; ++i) {
    const int64_t h = shapes[2 * i], w = shapes[2 * i + 1];
    SHDR_REQUIRE(h > 0 && w > 0, SHDR_E_SHAPE, "%s: file %d is %lld x %lld (H x W): sizes must be positive", what, i, (long long)h, (long long)w);
    SHDR_REQUIRE(w <= kMaxWidth && h <= (1 << 29), SHDR_E_SHAPE, "%s: file %d is %lld x %lld (H x W), the limits are 2^29 x %d", what, i,
                 (long long)h, (long long)w, kMaxWidth);
    const int64_t size = src_off[i + 1] - src_off[i];
    SHDR_REQUIRE(size >= 0, SHDR_E_SHAPE, "%s: src_off decreases at file %d", what, i);
    SHDR_REQUIRE(size <= 0x7fffffff, SHDR_E_SHAPE, "%s: file %d holds %lld bytes, the limit is 2^31 - 1", what, i, (long long)size);
    const int64_t ch = chunks_of(size, (int)w);
    p->rows += h;
    p->nodes += cap_of((int)h, (int)w) + 1;
    p->chunks += ch;
    if (ch > p->max_chunks) p->max_chunks = ch;
    p->out_bytes += 4 * h * w;
  }
  SHDR_REQUIRE(src_bytes < 0 || src_off[n] <= src_bytes, SHDR_E_SHAPE, "%s: src_off ends at %lld, the buffer holds %lld bytes", what,
               (long long)src_off[n], (long long)src_bytes);
  SHDR_REQUIRE(p->rows < ((int64_t)1 << 31) && p->nodes < ((int64_t)1 << 31), SHDR_E_SHAPE,
               "%s: %lld scanlines in one call, the limit is 2^29", what, (long long)p->rows);
  return SHDR_OK;
}

}  // namespace

extern "C" int64_t shdr_rgbe_rle_decode_status(const uint8_t* data, int64_t size, int width, int height, uint8_t* rgbe, int* status,
                                               int* line, int64_t* stop) {
  if ((!data && size) || !rgbe || !status || !line || !stop || size < 0 || width <= 0 || height <= 0) {
    shdr::set_error("rgbe_rle_decode_status: bad arguments");
    return -1;
  }
  return shdr_rle_dec::decode_serial(data, size, width, height, rgbe, status, line, stop);
}

extern "C" int shdr_rgbe_rle_decode_batch_sizes(const int32_t* shapes, const int64_t* src_off, int n_files, int64_t* out_bytes,
                                                int64_t* workspace_bytes) {
  Plan p;
  if (int rc = make_plan("rgbe_rle_decode_batch_sizes", shapes, src_off, n_files, -1, &p)) return rc;
  if (out_bytes) *out_bytes = p.out_bytes;
  if (workspace_bytes) *workspace_bytes = carve(nullptr, n_files, p.rows, p.nodes, p.chunks).bytes;
  return SHDR_OK;
}

extern "C" int shdr_rgbe_rle_decode_batch(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* src_off_dev,
                                          const int32_t* shapes, const int32_t* shapes_dev, int n_files, uint8_t* out, int64_t out_bytes,
                                          int64_t* out_off_dev, void* workspace, int64_t workspace_bytes, int32_t* status, int32_t* line,
                                          int64_t* consumed, void* stream, float* stage_ms) {
  const char* what = "rgbe_rle_decode_batch";
  SHDR_REQUIRE(src_off_dev && shapes_dev && out && out_off_dev && workspace && status && line && consumed, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(src_bytes >= 0 && (src || !src_bytes), SHDR_E_NULL, "%s: null buffer", what);
  Plan p;
  if (int rc = make_plan(what, shapes, src_off, n_files, src_bytes, &p)) return rc;
  SHDR_REQUIRE(out_bytes >= p.out_bytes, SHDR_E_SHAPE, "%s: output buffer too small (%lld < %lld)", what, (long long)out_bytes,
               (long long)p.out_bytes);
  const DecWorkspace w = carve(workspace, n_files, p.rows, p.nodes, p.chunks);
  SHDR_REQUIRE(workspace_bytes >= w.bytes, SHDR_E_SHAPE, "%s: the workspace holds %lld bytes, %lld are needed", what,
               (long long)workspace_bytes, (long long)w.bytes);
  SHDR_REQUIRE((reinterpret_cast<uintptr_t>(src_off_dev) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out_off_dev) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(consumed) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(line) & 3u) == 0 && (reinterpret_cast<uintptr_t>(shapes_dev) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(out) & 3u) == 0 && shdr::aligned16(workspace),
               SHDR_E_ALIGN, "%s: the offset tables and `consumed` must be 8-byte aligned, `status`, `line`, the shape table and out 4-byte, the workspace 16-byte",
               what);
  hipStream_t st = shdr::stream_of(stream);
  shdr::StageTimer<SHDR_RGBE_DEC_STAGES> timer(stage_ms, st);
  hipLaunchKernelGGL(dec_setup_kernel, dim3(1), dim3(64), 0, st, shapes_dev, src_off_dev, src_bytes, n_files, w.rowstart, w.nodeoff,
                     w.chunkoff, w.ncand, out_off_dev);
  if (p.max_chunks > 0) {
    const dim3 grid((unsigned)p.max_chunks, (unsigned)n_files);
    hipLaunchKernelGGL(dec_count_kernel, grid, dim3(256), 0, st, src, src_bytes, src_off_dev, shapes_dev, w.chunkoff, w.chunkcnt);
    hipLaunchKernelGGL(dec_compact_kernel, grid, dim3(256), 0, st, src, src_bytes, src_off_dev, shapes_dev, w.chunkoff, w.chunkcnt,
                       w.nodeoff, w.ncand, w.n_pos);
  }
  timer.mark();
  hipLaunchKernelGGL(dec_parse_kernel, dim3((unsigned)p.nodes), dim3(64), 0, st, src, src_bytes, src_off_dev, shapes_dev, n_files, w.nodeoff,
                     w.ncand, w.n_pos, w.n_end, w.n_fail, w.n_rel, w.n_stop, w.n_flat, w.n_next[0], w.n_len[0], w.n_comp);
  timer.mark();
  hipLaunchKernelGGL(dec_rank_kernel, dim3((unsigned)n_files), dim3(1024), 0, st, shapes_dev, w.rowstart, w.nodeoff, w.ncand, w.n_pos,
                     w.n_end, w.n_fail, w.n_rel, w.n_stop, w.n_flat, w.n_mark, w.n_row, w.n_next[0], w.n_next[1], w.n_len[0], w.n_len[1],
                     w.rowdesc, status, line, consumed);
  timer.mark();
  hipLaunchKernelGGL(dec_expand_kernel, dim3((unsigned)p.rows), dim3(256), 0, st, src, src_bytes, src_off_dev, shapes_dev, n_files,
                     w.rowstart, w.nodeoff, w.n_comp, w.rowdesc, out_off_dev, out, out_bytes);
  timer.mark();
  return shdr::check_launch(what);
}
