// Sanitizer sweep of the PNG writer's host twin (csrc/png.h) on the host: the kernels' filters, segment framing and checksum algebra
// are this header, so what holds here is what stands behind the device's reads of an image.  Stand-alone, no HIP, not part of the
// library or of the test suite:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I singlehdr-tf2_amd/csrc tools/png_enc_sweep.cpp -o /tmp/png_enc_sweep
//     /tmp/png_enc_sweep
//
// 3252 random images -- widths 1 .. 130 and a few above 21 840 (with C = 3 or 4: rows longer than a segment), 1 .. 40 rows, C of 1, 3 and 4, five
// kinds of content, every filter option, both deflate choices -- are encoded from a heap block of exactly H W C bytes into heap
// blocks of exactly the bound, of exactly the file's size and of one byte less (which must write nothing), so a read one byte outside
// the image or a write one byte outside the file is an AddressSanitizer report.  Every file is taken apart again here: the chunks and
// their CRCs (against a bitwise CRC and against the lanes' slice-and-shift form, crc_shift), the IDAT data through the project's own
// inflate (csrc/inflate.h), the Adler-32 (against adler_combine over the segments), and an unfilter written below.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflate.h"
#include "png.h"

namespace {

using namespace shdr_png;

long long g_runs = 0, g_in = 0, g_out = 0, g_idat = 0;
uint32_t g_state = 2024;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u, g_state >> 8; }

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "line %d: %s fails (run %lld)\n", __LINE__, #cond, g_runs); \
      abort();                                                             \
    }                                                                      \
  } while (0)

uint32_t crc_bitwise(const uint8_t* p, int64_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return ~c;
}

// what a block of `lanes` lanes computes in png_frame_kernel
uint32_t crc_sliced(const uint8_t* p, int64_t len, int lanes) {
  const uint32_t* table = crc_table_host();
  const int64_t per = (len + lanes - 1) / lanes;
  uint32_t all = 0;
  for (int t = 0; t < lanes; ++t) {
    const int64_t lo = per * t < len ? per * t : len, hi = lo + per < len ? lo + per : len;
    all ^= crc_shift(crc_bytes(t == 0 ? 0xFFFFFFFFu : 0u, p + lo, hi - lo, table), len - hi);
  }
  return ~all;
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// the pixels of a filtered stream: PNG's reconstruction, written apart from png.h's filters
std::vector<uint8_t> unfilter(const std::vector<uint8_t>& s, int64_t h, int64_t w, int c, int want_type) {
  const int64_t n = w * c;
  std::vector<uint8_t> px((size_t)(h * n));
  for (int64_t y = 0; y < h; ++y) {
    const int type = s[(size_t)(y * (n + 1))];
    CHECK(type >= 0 && type <= 4 && (want_type == kAdaptive || type == want_type));
    const uint8_t* f = &s[(size_t)(y * (n + 1) + 1)];
    for (int64_t i = 0; i < n; ++i) {
      const int a = i >= c ? px[(size_t)(y * n + i - c)] : 0, b = y ? px[(size_t)((y - 1) * n + i)] : 0;
      const int cc = y && i >= c ? px[(size_t)((y - 1) * n + i - c)] : 0;
      int pred = 0;
      if (type == 1) pred = a;
      if (type == 2) pred = b;
      if (type == 3) pred = (a + b) / 2;
      if (type == 4) {
        const int p = a + b - cc, pa = abs(p - a), pb = abs(p - b), pc = abs(p - cc);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : cc);
      }
      px[(size_t)(y * n + i)] = (uint8_t)(f[i] + pred);
    }
  }
  return px;
}

void run(int64_t h, int64_t w, int c, int kind, int filter, int deflate) {
  const size_t bytes = (size_t)(h * w * c);
  uint8_t* src = static_cast<uint8_t*>(malloc(bytes));           // exact blocks: the redzones begin at src + bytes and dst + size
  const uint32_t period = 1 + rnd() % 61;
  for (size_t i = 0; i < bytes; ++i) {
    const size_t x = i / c % (size_t)w, y = i / c / (size_t)w;
    switch (kind) {
      case 0: src[i] = 0; break;
      case 1: src[i] = (uint8_t)(x * 3 + y * 5 + i % c * 40); break;
      case 2: src[i] = (uint8_t)rnd(); break;
      case 3: src[i] = (uint8_t)(x * x / 9 + x * y / 3 + rnd() % 3); break;
      default: src[i] = (uint8_t)(17 * (i % period)); break;
    }
  }
  const int64_t stream = stream_bytes(h, w, c), bound = file_bound(stream);
  uint8_t* big = static_cast<uint8_t*>(malloc((size_t)bound));
  int64_t need = 0;
  const int64_t size = encode_host(src, h, w, c, filter, deflate, big, bound, &need);
  CHECK(size > 0 && size == need && size <= bound);
  uint8_t* dst = static_cast<uint8_t*>(malloc((size_t)size));
  memset(dst, 0xAB, (size_t)size);
  CHECK(encode_host(src, h, w, c, filter, deflate, dst, size - 1, nullptr) == -2);
  for (int64_t i = 0; i < size; ++i) CHECK(dst[i] == 0xAB);      // one byte short: nothing written
  CHECK(encode_host(src, h, w, c, filter, deflate, dst, size, nullptr) == size);
  CHECK(!memcmp(dst, big, (size_t)size));
  // the chunks
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 13, 10, 26, 10};
  CHECK(!memcmp(dst, sig, 8));
  std::vector<uint8_t> z;
  int64_t at = 8, n_idat = 0;
  bool end = false;
  while (at < size) {
    CHECK(!end && at + 12 <= size);
    const int64_t len = be32(dst + at);
    CHECK(at + 12 + len <= size);
    const uint32_t crc = be32(dst + at + 8 + len);
    CHECK(crc == crc_bitwise(dst + at + 4, len + 4) && crc == crc_sliced(dst + at + 4, len + 4, 256) && crc == crc_sliced(dst + at + 4, len + 4, 7));
    if (!memcmp(dst + at + 4, "IHDR", 4)) {
      CHECK(at == 8 && len == 13 && be32(dst + 16) == (uint32_t)w && be32(dst + 20) == (uint32_t)h && dst[24] == 8 &&
            dst[25] == colour_type(c) && !dst[26] && !dst[27] && !dst[28]);
    } else if (!memcmp(dst + at + 4, "IDAT", 4)) {
      z.insert(z.end(), dst + at + 8, dst + at + 8 + len);
      ++n_idat;
    } else {
      CHECK(!memcmp(dst + at + 4, "IEND", 4) && len == 0);
      end = true;
    }
    at += 12 + len;
  }
  CHECK(end && at == size && n_idat == segments(stream));
  // the zlib stream, the checksum, the pixels
  std::vector<uint8_t> back((size_t)stream);
  int status = -1;
  CHECK(shdr_inflate::inflate_host(z.data(), (int64_t)z.size(), back.data(), stream, &status) == stream && status == 0);
  uint32_t adler = 1;
  for (int64_t lo = 0; lo < stream; lo += kPngSegment) {
    const int64_t n = stream - lo < kPngSegment ? stream - lo : kPngSegment;
    adler = adler_combine(adler, shdr_deflate::adler32_host(back.data() + lo, n), n);
  }
  CHECK(adler == be32(z.data() + z.size() - 4) && adler == shdr_deflate::adler32_host(back.data(), stream));
  const std::vector<uint8_t> px = unfilter(back, h, w, c, filter);
  CHECK(!memcmp(px.data(), src, bytes));
  ++g_runs;
  g_in += (long long)bytes;
  g_out += size;
  g_idat += n_idat;
  free(dst);
  free(big);
  free(src);
}

}  // namespace

int main() {
  const int cs[3] = {1, 3, 4};
  int k = 0;
  for (int round = 0; round < 270; ++round) {
    for (int filter = 0; filter <= kAdaptive; ++filter) {
      for (int deflate = 0; deflate < 2; ++deflate, ++k) {
        const int c = cs[rnd() % 3];
        run(1 + rnd() % 40, 1 + rnd() % 130, c, k % 5, filter, deflate);
      }
    }
  }
  for (int filter = 0; filter <= kAdaptive; ++filter) {                       // widths above 21 840
    for (int deflate = 0; deflate < 2; ++deflate, ++k) run(1 + k % 3, 21841 + rnd() % 300, cs[k % 3], k % 5, filter, deflate);
  }
  printf("%lld images, %lld IDAT chunks, %lld bytes in, %lld bytes out\n", g_runs, g_idat, g_in, g_out);
  return 0;
}
