// Sanitizer sweep of the inflate core (csrc/inflate.h) on the host: the kernel's bounds logic is this header, so what holds here is what
// stands behind feeding malformed bytes to the device.  Stand-alone, no HIP, not part of the library or of the test suite:
//
//     python tests/deflate_synth.py --dump /tmp/zz
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I singlehdr-tf2_amd/csrc tools/inflate_sweep.cpp -o /tmp/inflate_sweep
//     /tmp/inflate_sweep /tmp/zz
//
// Every <name>.<want>.zz of the directory is decoded with a capacity of exactly `want`; streams of up to kSmall bytes are also decoded
// with every single bit flipped and cut at every length.  Source and destination are heap blocks of exactly n and `want` bytes, so a
// read or write one byte outside either is an AddressSanitizer report.  The program itself asserts only that `written` stays within
// the capacity; it prints how many decodes ran and how they ended.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <string>
#include <vector>

#include "inflate.h"

namespace {

constexpr size_t kSmall = 400;
long long g_runs = 0, g_by_status[shdr_inflate::kStatusCount] = {};

int decode(const std::vector<uint8_t>& stream, size_t n, int64_t want) {
  uint8_t* src = static_cast<uint8_t*>(malloc(n ? n : 1));       // exact blocks: the redzones begin at src + n and dst + want
  uint8_t* dst = static_cast<uint8_t*>(malloc(want ? want : 1));
  if (n) memcpy(src, stream.data(), n);
  int status = -1;
  const int64_t written = shdr_inflate::inflate_host(n ? src : nullptr, (int64_t)n, want ? dst : nullptr, want, &status);
  if (written < 0 || written > want || status < 0 || status >= shdr_inflate::kStatusCount) {
    fprintf(stderr, "written %lld of capacity %lld, status %d\n", (long long)written, (long long)want, status);
    abort();
  }
  ++g_runs;
  ++g_by_status[status];
  free(src);
  free(dst);
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s DIR   (of python tests/deflate_synth.py --dump DIR)\n", argv[0]);
    return 2;
  }
  DIR* dir = opendir(argv[1]);
  if (!dir) {
    perror(argv[1]);
    return 2;
  }
  int files = 0, swept = 0;
  while (dirent* e = readdir(dir)) {
    const std::string name = e->d_name;
    if (name.size() < 4 || name.substr(name.size() - 3) != ".zz") continue;
    const size_t dot = name.rfind('.', name.size() - 4);
    if (dot == std::string::npos) continue;
    const int64_t want = atoll(name.c_str() + dot + 1);
    FILE* f = fopen((std::string(argv[1]) + "/" + name).c_str(), "rb");
    if (!f) continue;
    std::vector<uint8_t> stream;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) stream.insert(stream.end(), buf, buf + got);
    fclose(f);
    ++files;
    decode(stream, stream.size(), want);
    if (stream.size() > kSmall) continue;
    ++swept;
    for (size_t cut = 0; cut < stream.size(); ++cut) decode(stream, cut, want);
    for (size_t bit = 0; bit < 8 * stream.size(); ++bit) {
      stream[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
      decode(stream, stream.size(), want);
      stream[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
    }
  }
  closedir(dir);
  printf("%d streams (%d swept bit by bit and cut by cut), %lld decodes\n", files, swept, g_runs);
  for (int s = 0; s < shdr_inflate::kStatusCount; ++s)
    if (g_by_status[s]) printf("  status %2d: %lld\n", s, g_by_status[s]);
  return files ? 0 : 1;
}
