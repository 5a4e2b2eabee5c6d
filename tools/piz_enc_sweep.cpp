// Sanitizer sweep of the PIZ encoder's rules (csrc/piz.h) on the host: random chunks through encode_host and back through decode_host.
// Stand-alone, no HIP, not part of the library or of the test suite:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I singlehdr-tf2_amd/csrc tools/piz_enc_sweep.cpp -o /tmp/piz_enc_sweep
//     /tmp/piz_enc_sweep [chunks, default 3000] [seed, default 1]
//
// Widths 1 .. 130, rows 1 .. 32, one to five channels of 1 or 2 words, and 1 .. 65536 distinct values per chunk (drawn so that small
// alphabets, hence long stretches and short tables, are as frequent as large ones), some with stretches laid in.  Source, destination
// and every table are heap blocks of exactly their sizes -- the destination exactly encode_bound, and once more exactly the bytes
// written, and once one byte less (which must be refused with nothing written) -- so a read or write one byte outside any of them is an
// AddressSanitizer report.  The program asserts decode_host(encode_host(raw)) == raw and prints what it ran.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "piz.h"

namespace {

using namespace shdr_piz;

uint64_t g_state = 1;
uint32_t rnd() {                                                 // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
uint32_t below(uint32_t n) { return (uint32_t)(((uint64_t)rnd() * n) >> 32); }

struct Enc {
  EncWork w;
  explicit Enc(int64_t values) {
    w.words = static_cast<uint32_t*>(malloc(4 * kBitmapWords));
    w.before = static_cast<uint32_t*>(malloc(4 * kBitmapWords));
    w.values = static_cast<uint16_t*>(malloc(2 * values));
    w.freq = static_cast<uint32_t*>(malloc(4 * kSymbols));
    w.keys = static_cast<uint64_t*>(malloc(8 * kSymbols));
    w.weight = static_cast<uint32_t*>(malloc(4 * kSymbols));
    w.made = static_cast<uint32_t*>(malloc(4 * kSymbols));
    w.parent = static_cast<uint32_t*>(malloc(4 * 2 * kSymbols));
    w.lens = static_cast<uint8_t*>(malloc(kSymbols));
    w.code = static_cast<uint64_t*>(malloc(8 * kSymbols));
  }
  ~Enc() {
    free(w.words); free(w.before); free(w.values); free(w.freq); free(w.keys);
    free(w.weight); free(w.made); free(w.parent); free(w.lens); free(w.code);
  }
};

void fail(const char* what, int width, int rows, int n_chan, uint32_t distinct) {
  fprintf(stderr, "%s: width %d, rows %d, %d channels, %u distinct values\n", what, width, rows, n_chan, distinct);
  abort();
}

}  // namespace

int main(int argc, char** argv) {
  const long chunks = argc > 1 ? atol(argv[1]) : 3000;
  g_state = argc > 2 ? strtoull(argv[2], nullptr, 10) | 1 : 1;
  long long bytes_in = 0, bytes_out = 0, coded = 0, wide = 0;
  for (long it = 0; it < chunks; ++it) {
    const int width = 1 + (int)below(130), rows = 1 + (int)below(32), n_chan = 1 + (int)below(5);
    std::vector<int32_t> words(n_chan);
    for (int c = 0; c < n_chan; ++c) words[c] = 1 + (int)below(2);
    const int64_t values = chunk_values(width, rows, words.data(), n_chan);
    if (values <= 0) fail("bad shape", width, rows, n_chan, 0);
    const uint32_t distinct = 1u + below(1u << (1 + below(16)));   // 1 .. 2^k for k = 1 .. 16: 1 .. 65536
    std::vector<uint16_t> alphabet(distinct);
    for (uint32_t i = 0; i < distinct; ++i) alphabet[i] = distinct > 60000 ? (uint16_t)i : (uint16_t)rnd();
    const uint32_t repeat = below(4) ? 0 : 1 + below(600);         // one chunk in four holds stretches in its scanlines
    uint8_t* raw = static_cast<uint8_t*>(malloc(2 * values));
    uint16_t v = 0;
    for (int64_t i = 0; i < values; ++i) {
      if (!repeat || below(repeat) == 0) v = alphabet[below(distinct)];
      raw[2 * i] = (uint8_t)v;
      raw[2 * i + 1] = (uint8_t)(v >> 8);
    }
    Enc e(values);
    const int64_t bound = encode_bound(values);
    uint8_t* big = static_cast<uint8_t*>(malloc(bound));
    const int64_t n = encode_host(raw, width, rows, words.data(), n_chan, big, bound, e.w);
    if (n <= 0 || n > bound) fail("encode_host refused the bound", width, rows, n_chan, distinct);
    uint8_t* exact = static_cast<uint8_t*>(malloc(n));
    if (encode_host(raw, width, rows, words.data(), n_chan, exact, n, e.w) != n || memcmp(big, exact, n)) fail("exact capacity", width, rows, n_chan, distinct);
    if (n > 1) {
      uint8_t* tight = static_cast<uint8_t*>(malloc(n - 1));
      memset(tight, 0xA5, n - 1);
      if (encode_host(raw, width, rows, words.data(), n_chan, tight, n - 1, e.w) != -2) fail("one byte less was accepted", width, rows, n_chan, distinct);
      for (int64_t i = 0; i < n - 1; ++i)
        if (tight[i] != 0xA5) fail("refused, but written", width, rows, n_chan, distinct);
      free(tight);
    }
    uint8_t* back = static_cast<uint8_t*>(malloc(2 * values));
    HostWork d;
    d.lens = static_cast<uint8_t*>(malloc(kSymbols));
    d.sorted = static_cast<uint16_t*>(malloc(2 * kSymbols));
    d.fast = static_cast<uint32_t*>(malloc(4 << kFastBits));
    d.lut = static_cast<uint16_t*>(malloc(2 * kLutSize));
    d.values = static_cast<uint16_t*>(malloc(2 * values));
    const int status = decode_host(exact, n, width, rows, words.data(), n_chan, back, d);
    if (status != kOk) fail("decode_host refused the encoder's bytes", width, rows, n_chan, distinct);
    if (memcmp(back, raw, 2 * values)) fail("round trip differs", width, rows, n_chan, distinct);
    bytes_in += 2 * values;
    bytes_out += n;
    coded += n < 2 * values;
    wide += distinct > 16384;
    free(d.values); free(d.lut); free(d.fast); free(d.sorted); free(d.lens);
    free(back); free(exact); free(big); free(raw);
  }
  printf("%ld chunks, %lld scanline bytes -> %lld PIZ bytes, %lld chunks strictly smaller, %lld drawn from more than 16384 values: clean\n", chunks,
         bytes_in, bytes_out, coded, wide);
  return 0;
}
