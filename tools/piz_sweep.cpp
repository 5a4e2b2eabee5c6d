// Sanitizer sweep of the PIZ rules (csrc/piz.h) on the host: the kernels' bounds logic for the stream is this header, so what holds
// here is what stands behind feeding malformed bytes to the device.  Stand-alone, no HIP, not part of the library or of the test suite:
//
//     python tests/piz_cases.py --dump /tmp/pz
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I singlehdr-tf2_amd/csrc tools/piz_sweep.cpp -o /tmp/piz_sweep
//     /tmp/piz_sweep /tmp/pz
//
// Every <name>.<width>.<rows>.<words>.piz of the directory (<words>: one digit per channel) is decoded; chunks of up to kSmall bytes
// are also decoded with every single bit flipped and cut at every length -- the mutations of tests/test_piz_host.py.  Source,
// destination and every table are heap blocks of exactly their sizes, so a read or write one byte outside any of them is an
// AddressSanitizer report.  The program itself asserts that every decode ends in a status and that a refused chunk leaves its
// destination untouched; it prints how many decodes ran and how they ended.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <string>
#include <vector>

#include "piz.h"

namespace {

using namespace shdr_piz;

constexpr size_t kSmall = 600;
long long g_runs = 0, g_by_status[kStatusCount] = {};

int decode(const std::vector<uint8_t>& chunk, size_t n, int width, int rows, const std::vector<int32_t>& words) {
  const int64_t values = chunk_values(width, rows, words.data(), (int)words.size());
  if (values <= 0) {
    fprintf(stderr, "bad shape %d x %d\n", width, rows);
    abort();
  }
  uint8_t* src = static_cast<uint8_t*>(malloc(n ? n : 1));       // exact blocks: the redzones begin at src + n, dst + 2 * values, ...
  uint8_t* dst = static_cast<uint8_t*>(malloc(2 * values));
  if (n) memcpy(src, chunk.data(), n);
  memset(dst, 0xA5, 2 * values);
  HostWork w;
  w.lens = static_cast<uint8_t*>(malloc(kSymbols));
  w.sorted = static_cast<uint16_t*>(malloc(2 * kSymbols));
  w.fast = static_cast<uint32_t*>(malloc(4 << kFastBits));
  w.lut = static_cast<uint16_t*>(malloc(2 * kLutSize));
  w.values = static_cast<uint16_t*>(malloc(2 * values));
  const int status = decode_host(src, (int64_t)n, width, rows, words.data(), (int)words.size(), dst, w);
  if (status < 0 || status >= kStatusCount) {
    fprintf(stderr, "status %d\n", status);
    abort();
  }
  if (status != kOk)
    for (int64_t i = 0; i < 2 * values; ++i)
      if (dst[i] != 0xA5) {
        fprintf(stderr, "status %d, but byte %lld of the destination was written\n", status, (long long)i);
        abort();
      }
  ++g_runs;
  ++g_by_status[status];
  free(w.values);
  free(w.lut);
  free(w.fast);
  free(w.sorted);
  free(w.lens);
  free(src);
  free(dst);
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s DIR   (of python tests/piz_cases.py --dump DIR)\n", argv[0]);
    return 2;
  }
  DIR* dir = opendir(argv[1]);
  if (!dir) {
    perror(argv[1]);
    return 2;
  }
  int files = 0, swept = 0, refused = 0;
  while (dirent* e = readdir(dir)) {
    const std::string name = e->d_name;
    if (name.size() < 5 || name.substr(name.size() - 4) != ".piz") continue;
    // <name>.<width>.<rows>.<words>.piz
    size_t d3 = name.size() - 4, d2 = name.rfind('.', d3 - 1);
    if (d2 == std::string::npos || d2 == 0) continue;
    const size_t d1 = name.rfind('.', d2 - 1);
    if (d1 == std::string::npos || d1 == 0) continue;
    const size_t d0 = name.rfind('.', d1 - 1);
    if (d0 == std::string::npos) continue;
    const int width = atoi(name.c_str() + d0 + 1), rows = atoi(name.c_str() + d1 + 1);
    std::vector<int32_t> words;
    for (size_t i = d2 + 1; i < d3; ++i) words.push_back(name[i] - '0');
    FILE* f = fopen((std::string(argv[1]) + "/" + name).c_str(), "rb");
    if (!f) continue;
    std::vector<uint8_t> chunk;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) chunk.insert(chunk.end(), buf, buf + got);
    fclose(f);
    ++files;
    if (decode(chunk, chunk.size(), width, rows, words) != kOk) ++refused;
    if (chunk.size() > kSmall) continue;
    ++swept;
    for (size_t cut = 0; cut < chunk.size(); ++cut) decode(chunk, cut, width, rows, words);
    for (size_t bit = 0; bit < 8 * chunk.size(); ++bit) {
      chunk[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
      decode(chunk, chunk.size(), width, rows, words);
      chunk[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
    }
  }
  closedir(dir);
  printf("%d chunks (%d swept bit by bit and cut by cut), %lld decodes, %d of the unchanged chunks refused\n", files, swept, g_runs, refused);
  for (int s = 0; s < kStatusCount; ++s)
    if (g_by_status[s]) printf("  status %2d: %lld\n", s, g_by_status[s]);
  return files && !refused ? 0 : 1;
}
