// Sanitizer sweep of the LZ77 deflate encoder (csrc/deflate_lz.h) on the host: the kernels' parse, symbols and header are this header,
// so what holds here is what stands behind the device's reads of a chunk.  Stand-alone, no HIP, not part of the library or of the
// test suite:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I singlehdr-tf2_amd/csrc tools/deflate_lz_sweep.cpp -o /tmp/deflate_lz_sweep
//     /tmp/deflate_lz_sweep
//
// Chunks of every length 1 .. 600 and of some longer ones, of six kinds (one value, a period, few values, a slow ramp, noise, a block
// repeated far back), are encoded from a heap block of exactly n bytes into a heap block of exactly the stream's size, so a read one
// byte outside the chunk or a write one byte outside the stream is an AddressSanitizer report; then once more with a capacity one
// short, which must write nothing.  Every stream is decoded by the project's own inflate (csrc/inflate.h) and compared.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deflate_lz.h"
#include "inflate.h"

namespace {

long long g_runs = 0, g_in = 0, g_out = 0;
uint32_t g_state = 12345;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u, g_state >> 8; }

std::vector<uint8_t> make(int kind, size_t n) {
  std::vector<uint8_t> v(n);
  const uint32_t period = 1 + rnd() % 97;
  for (size_t i = 0; i < n; ++i) {
    switch (kind) {
      case 0: v[i] = 0x80; break;
      case 1: v[i] = (uint8_t)(31 * (i % period)); break;
      case 2: v[i] = (uint8_t)(126 + rnd() % 5); break;
      case 3: v[i] = (uint8_t)(i / 41 + rnd() % 2); break;
      case 4: v[i] = (uint8_t)rnd(); break;
      default: v[i] = i < 64 || i + 64 >= n ? (uint8_t)(7 * (i % 64) + 1) : 0xEE; break;   // the first 64 bytes come again at the end
    }
  }
  return v;
}

void run(const std::vector<uint8_t>& chunk) {
  const int64_t n = (int64_t)chunk.size();
  uint8_t* src = static_cast<uint8_t*>(malloc(chunk.size()));    // exact blocks: the redzones begin at src + n and dst + need
  memcpy(src, chunk.data(), chunk.size());
  uint8_t probe[1];
  int64_t need = 0;
  if (shdr_deflate_lz::encode_host(src, n, probe, 0, &need) != -2 || need < shdr_deflate_lz::kHeaderBytes + 4) abort();
  uint8_t* dst = static_cast<uint8_t*>(malloc((size_t)need));
  memset(dst, 0xAB, (size_t)need);
  if (shdr_deflate_lz::encode_host(src, n, dst, need - 1, nullptr) != -2) abort();
  for (int64_t i = 0; i < need; ++i)
    if (dst[i] != 0xAB) abort();                                 // one byte short: nothing written
  if (shdr_deflate_lz::encode_host(src, n, dst, need, nullptr) != need) abort();
  uint32_t* tokens = static_cast<uint32_t*>(malloc(4 * chunk.size()));
  std::vector<uint32_t> table(shdr_deflate_lz::kHashSlots);
  shdr_deflate_lz::parse_host(src, n, tokens, table.data());
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!tokens[i]) continue;
    if (i != at) abort();                                        // the tokens tile the chunk
    at += shdr_deflate_lz::token_is_literal(tokens[i]) ? 1 : shdr_deflate_lz::token_length(tokens[i]);
  }
  if (at != n) abort();
  uint8_t* back = static_cast<uint8_t*>(malloc(chunk.size()));
  int status = -1;
  if (shdr_inflate::inflate_host(dst, need, back, n, &status) != n || status != 0 || memcmp(back, src, chunk.size())) {
    fprintf(stderr, "a chunk of %lld bytes does not come back (status %d)\n", (long long)n, status);
    abort();
  }
  ++g_runs;
  g_in += n;
  g_out += need;
  free(back);
  free(tokens);
  free(dst);
  free(src);
}

}  // namespace

int main() {
  for (int kind = 0; kind < 6; ++kind) {
    for (size_t n = 1; n <= 600; ++n) run(make(kind, n));
    for (size_t n : {1023u, 1024u, 1025u, 4097u, 32767u, 32768u, 32769u, 32832u, 32833u, 70001u, 400003u}) run(make(kind, n));
  }
  printf("%lld chunks, %lld bytes in, %lld bytes out\n", g_runs, g_in, g_out);
  return 0;
}
