// Sanitizer sweep of the baseline-JPEG writer's host twin (csrc/jpeg_enc.h) on the CPU: the kernels' rules and bounds logic are this
// header, so what holds here is what stands behind them.  Stand-alone, no HIP, no Python at run time, not part of the library or of the
// test suite:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I singlehdr-tf2_amd/csrc tools/jpeg_enc_sweep.cpp -o /tmp/jpeg_enc_sweep
//     /tmp/jpeg_enc_sweep [runs]
//
// Random sizes (1 .. 70, and a few up to 300 wide or high), layouts, qualities, restart intervals and contents (noise, flat, ramp).
// Every image is transformed and coded into heap blocks of EXACTLY the stated sizes, so a read or write one byte outside any of them is
// an AddressSanitizer report; then coded again with a capacity one byte short, half, and zero, which must fail and leave the block's
// prefix as it was; then its coefficient arena is made hostile -- random int16 values, the extremes, values just inside and outside the
// baseline range -- and coded once more: either the range error names a block that holds such a value, or the scan decodes back
// (a decoder written here from T.81, sharing only the tables) to the arena.  Every good scan is decoded back as well.  The program
// asserts all that and prints how many encodes ran.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "jpeg_enc.h"

namespace {

using namespace jpegenc;

long long g_encodes = 0, g_short = 0, g_hostile_ok = 0, g_hostile_refused = 0;

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 16);
}
int uniform(int lo, int hi) { return lo + (int)(rnd() % (uint32_t)(hi - lo + 1)); }

void die(const char* what, const Image& im) {
  fprintf(stderr, "%s: %d x %d layout %d quality %d restart %d\n", what, im.height, im.width, im.layout, im.quality, im.restart);
  abort();
}

// the scan decoded back to an arena: unstuffing, RSTn markers in order, the four standard tables
bool decode_scan(const uint8_t* s, int64_t n, const Image& im, std::vector<int16_t>* out) {
  const Geometry g = geometry(im);
  out->assign((size_t)g.blocks * 64, 0);
  int64_t pos = 0;
  uint32_t acc = 0;
  int nbits = 0;
  auto bit = [&]() -> int {
    if (nbits == 0) {
      if (pos >= n) return -1;
      acc = s[pos++];
      if (acc == 0xFF) {
        if (pos >= n || s[pos] != 0) return -1;
        ++pos;
      }
      nbits = 8;
    }
    return (int)(acc >> --nbits) & 1;
  };
  static std::unordered_map<uint32_t, int> by_code[4];             // length << 16 | code -> symbol
  if (by_code[0].empty())
    for (int t = 0; t < 4; ++t)
      for (int sym = 0; sym < 256; ++sym)
        if (kCodes.t[t].entry[sym]) by_code[t][kCodes.t[t].entry[sym]] = sym;
  auto symbol = [&](int t) -> int {
    uint32_t code = 0;
    for (int len = 1; len <= 16; ++len) {
      const int b = bit();
      if (b < 0) return -1;
      code = code << 1 | (uint32_t)b;
      const auto it = by_code[t].find((uint32_t)len << 16 | code);
      if (it != by_code[t].end()) return it->second;
    }
    return -1;
  };
  auto receive = [&](int sz, int* v) -> bool {
    int x = 0;
    for (int i = 0; i < sz; ++i) {
      const int b = bit();
      if (b < 0) return false;
      x = x << 1 | b;
    }
    *v = sz == 0 ? 0 : (x < (1 << (sz - 1)) ? x - (1 << sz) + 1 : x);
    return true;
  };
  int pred[3] = {0, 0, 0};
  for (int64_t b = 0; b < g.blocks; ++b) {
    const int64_t seg = segment_of_block(g, im.restart, b);
    if (b > 0 && b == segment_first_block(g, im.restart, seg)) {
      for (int i = 0; i < nbits; ++i)
        if (!((acc >> i) & 1)) return false;                       // the padding is 1-bits
      nbits = 0;
      if (pos + 2 > n || s[pos] != 0xFF || s[pos + 1] != rst_marker(seg - 1)) return false;
      pos += 2;
      pred[0] = pred[1] = pred[2] = 0;
    }
    const int k = (int)(b % g.nbm);
    const int comp = k < g.hv ? 0 : k - g.hv + 1;
    int16_t* zz = out->data() + b * 64;
    int sz = symbol(comp ? 2 : 0), v = 0;
    if (sz < 0 || sz > 11 || !receive(sz, &v)) return false;
    pred[comp] += v;
    zz[0] = (int16_t)pred[comp];
    for (int i = 1; i < 64;) {
      const int rs = symbol(comp ? 3 : 1);
      if (rs < 0) return false;
      if (rs == 0) break;
      if (rs == 0xF0) { i += 16; continue; }
      i += rs >> 4;
      if (i > 63 || !receive(rs & 15, &v)) return false;
      zz[i++] = (int16_t)v;
    }
  }
  for (int i = 0; i < nbits; ++i)
    if (!((acc >> i) & 1)) return false;
  return pos == n;
}

bool in_range(const int16_t* coef, const Image& im, int64_t* first_bad) {
  const Geometry g = geometry(im);
  for (int64_t b = 0; b < g.blocks; ++b) {
    const int64_t pb = pred_block(g, im.restart, b);
    const int diff = coef[b * 64] - (pb < 0 ? 0 : coef[pb * 64]);
    bool bad = diff > 2047 || diff < -2047;
    for (int k = 1; k < 64; ++k) bad = bad || coef[b * 64 + k] > 1023 || coef[b * 64 + k] < -1023;
    if (bad) {
      *first_bad = b;
      return false;
    }
  }
  return true;
}

void one(const Image& im, int content) {
  const Geometry g = geometry(im);
  const int64_t npix = (int64_t)im.height * im.width * 3;
  uint8_t* rgb = static_cast<uint8_t*>(malloc((size_t)npix));      // exact blocks: the redzone begins right behind them
  for (int64_t i = 0; i < npix; ++i)
    rgb[i] = content == 0 ? (uint8_t)rnd() : content == 1 ? (uint8_t)(im.quality * 2) : (uint8_t)((i / 3 % im.width) * 255 / im.width);
  int16_t* coef = static_cast<int16_t*>(malloc((size_t)g.blocks * 128));
  transform_host(rgb, im, coef);
  // the whole file into a block of the bound, then into one of exactly its size
  const int64_t bound = out_bound(g);
  uint8_t* big = static_cast<uint8_t*>(malloc((size_t)bound));
  int64_t bad = -1;
  const int64_t n = encode_host(rgb, im, coef, big, bound, &bad);
  ++g_encodes;
  if (n < header_length(im) + 3 || n > bound) die("the file's size is outside its bounds", im);
  uint8_t header[kHeaderMax];
  if (compose_header(im, header) != header_length(im) || memcmp(big, header, (size_t)header_length(im)) != 0) die("header", im);
  if (big[n - 2] != 0xFF || big[n - 1] != 0xD9) die("no EOI", im);
  std::vector<int16_t> back;
  if (!decode_scan(big + header_length(im), n - header_length(im) - 2, im, &back) || memcmp(back.data(), coef, (size_t)g.blocks * 128) != 0)
    die("the scan does not decode back to the coefficients", im);
  uint8_t* exact = static_cast<uint8_t*>(malloc((size_t)n));
  if (encode_host(rgb, im, coef, exact, n, &bad) != n || memcmp(exact, big, (size_t)n) != 0) die("exact capacity", im);
  ++g_encodes;
  free(exact);
  // capacities that are too small: an error, nothing past the capacity (the block ends there)
  const int64_t caps[4] = {n - 1, n / 2, 1, 0};
  for (int64_t cap : caps) {
    uint8_t* small = static_cast<uint8_t*>(malloc(cap ? (size_t)cap : 1));
    if (encode_host(rgb, im, coef, small, cap, &bad) != kCapacityError) die("a short capacity was accepted", im);
    if (cap > 0 && memcmp(small, big, (size_t)(cap < n - 2 ? cap : n - 2)) != 0) die("a short capacity changed the bytes before it", im);   // (EOI is written whole or not at all)
    free(small);
    ++g_encodes;
    ++g_short;
  }
  // the entropy stage alone, one byte short
  const int64_t sn = n - header_length(im) - 2;
  {
    uint8_t* small = static_cast<uint8_t*>(malloc((size_t)(sn > 1 ? sn - 1 : 1)));
    if (entropy_host(coef, im, small, sn - 1, &bad) != kCapacityError) die("entropy stage: a short capacity was accepted", im);
    free(small);
    ++g_encodes;
    ++g_short;
  }
  // hostile arenas
  for (int round = 0; round < 3; ++round) {
    const int edits = round == 0 ? 1 : uniform(1, 40);
    for (int e = 0; e < edits; ++e) {
      static const int16_t values[] = {1023, -1023, 1024, -1024, 2047, -2047, 2048, -2048, 32767, -32768, 0, 1, -1};
      const int64_t at = (int64_t)(rnd() % (uint32_t)(g.blocks * 64));
      coef[at] = round == 2 ? (int16_t)rnd() : values[rnd() % (sizeof(values) / sizeof(values[0]))];
    }
    int64_t want_bad = -1;
    const bool ok = in_range(coef, im, &want_bad);
    const int64_t hn = entropy_host(coef, im, big, bound, &bad);
    ++g_encodes;
    if (ok) {
      ++g_hostile_ok;
      if (hn <= 0 || !decode_scan(big, hn, im, &back) || memcmp(back.data(), coef, (size_t)g.blocks * 128) != 0)
        die("a hostile arena inside the range does not decode back", im);
    } else {
      ++g_hostile_refused;
      if (hn != kRangeError || bad != want_bad) die("a coefficient outside the range was not refused at its block", im);
    }
  }
  free(big);
  free(coef);
  free(rgb);
}

}  // namespace

int main(int argc, char** argv) {
  const int runs = argc > 1 ? atoi(argv[1]) : 4000;
  for (int r = 0; r < runs; ++r) {
    Image im;
    const bool large = r % 50 == 49;
    im.height = large ? uniform(1, 300) : uniform(1, 70);
    im.width = large ? uniform(1, 300) : uniform(1, 70);
    im.layout = uniform(0, 2);
    im.quality = r % 7 == 0 ? (r % 2 ? 1 : 100) : uniform(1, 100);
    const Image probe = {im.height, im.width, im.layout, im.quality, 0, 0};
    const int mcus = (int)geometry(probe).mcus;
    const int kind = uniform(0, 4);
    im.restart = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? uniform(2, mcus + 2) : kind == 3 ? mcus : 65535;
    im.reserved = 0;
    if (!image_ok(im)) die("image_ok refuses a valid image", im);
    one(im, uniform(0, 2));
  }
  const Image bad[] = {{0, 8, 0, 50, 0, 0}, {8, 65536, 0, 50, 0, 0}, {8, 8, 3, 50, 0, 0}, {8, 8, -1, 50, 0, 0}, {8, 8, 0, 0, 0, 0},
                       {8, 8, 0, 101, 0, 0}, {8, 8, 0, 50, -1, 0}, {8, 8, 0, 50, 65536, 0}};
  for (const Image& im : bad)
    if (image_ok(im)) die("image_ok accepts an invalid image", im);
  printf("jpeg_enc_sweep: %lld encodes (%lld into short buffers, %lld hostile arenas coded, %lld refused), clean\n", g_encodes, g_short,
         g_hostile_ok, g_hostile_refused);
  return 0;
}
