// Sanitizer sweep of the JPEG scan preparation (csrc/jpeg_scan.h) on the host: the kernels' rules and bounds logic are this header, so
// what holds here is what stands behind feeding arbitrary bytes to the device.  Stand-alone, no HIP, no Python at run time, not part of
// the library or of the test suite:
//
//     python tests/jpeg_scan_ref.py --dump /tmp/scans
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I singlehdr-tf2_amd/csrc tools/jpeg_scan_sweep.cpp -o /tmp/jpeg_scan_sweep
//     /tmp/jpeg_scan_sweep /tmp/scans
//
// Every <name>.<seg_cap>.scan of the directory (the corpus of the tests) and 20000 random strings over a marker-rich alphabet are
// scanned and compacted with the stated seg_cap and with 1, with one fewer and one more than the markers they hold need -- so that
// files with more restart markers than slots, and with fewer, are always among them -- and compacted once more into an arena one
// byte short and into none.  Source, boundary array and arena are heap blocks of exactly the stated sizes, so a read or write one
// byte outside any of them is an AddressSanitizer report.  The program itself asserts that the report is consistent and that the arena
// holds the kept bytes of a serial pass of its own; it prints how many scans ran.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <string>
#include <vector>

#include "jpeg_scan.h"

namespace {

using namespace jpegscan;

long long g_runs = 0, g_no_end = 0, g_more = 0, g_fewer = 0, g_fill = 0;

void die(const char* what, const std::string& name) {
  fprintf(stderr, "%s: %s\n", name.c_str(), what);
  abort();
}

void run(const std::string& name, const std::vector<uint8_t>& bytes, int seg_cap) {
  const int64_t n = (int64_t)bytes.size();
  uint8_t* src = static_cast<uint8_t*>(malloc(n ? n : 1));        // exact blocks: the redzone begins at src + n
  if (n) memcpy(src, bytes.data(), n);
  const int64_t slots = seg_cap - 1;
  int64_t* bounds = static_cast<int64_t*>(malloc(slots ? 8 * slots : 1));
  Image im{0, n, 0, seg_cap, 0, 0, 0};
  int64_t tiles = 0;
  int bad = 0;
  if (check_images(&im, 1, n, slots, seg_cap, &tiles, &bad) != kOk || tiles != (n + kTile - 1) / kTile) die("descriptor refused", name);
  Report rep;
  scan_host(src, im, &rep, bounds);
  const int64_t stop = rep.end == kNone ? n : rep.end;
  if (rep.end < kNone || rep.end >= n || rep.kept < 0 || rep.kept > stop || rep.n_rst < 0 || 2 * (int64_t)rep.n_rst > stop ||
      (rep.end != kNone && (src[rep.end] != 0xFF || rep.end_marker != src[rep.end + 1])))
    die("inconsistent report", name);
  // the segments as jpeg.py lays them out: lengths from the boundaries, what follows the last filled slot in the last segment
  const int64_t filled = rep.n_rst < slots ? rep.n_rst : slots;
  std::vector<int64_t> length(seg_cap, 0);
  int64_t prev = 0;
  for (int64_t s = 0; s < filled; ++s) {
    if (bounds[s] < prev || bounds[s] > rep.kept) die("boundaries do not ascend", name);
    length[s] = bounds[s] - prev;
    prev = bounds[s];
  }
  for (int64_t s = filled; s < slots; ++s)
    if (bounds[s] != kNone) die("an unfilled slot was written", name);
  length[filled] = rep.kept - prev;
  std::vector<int32_t> dword(seg_cap);
  int64_t dwords = 0;
  for (int s = 0; s < seg_cap; ++s) {
    dword[s] = (int32_t)dwords;
    dwords += (length[s] + 3) / 4;
  }
  // what the arena must hold: a serial pass that knows nothing of byte_class
  std::vector<uint8_t> want(4 * dwords, 0xFF);
  {
    int64_t seg = 0, in_seg = 0;
    for (int64_t p = 0; p < stop; ++p) {
      if (src[p] == 0xFF && p + 1 < n && src[p + 1] >= 0xD0 && src[p + 1] <= 0xD7) {
        ++p;
        if (seg < filled) {
          ++seg;
          in_seg = 0;
        }
        continue;
      }
      if (src[p] == 0x00 && p > 0 && src[p - 1] == 0xFF) continue;
      want[4 * (int64_t)dword[seg] + in_seg++] = src[p];
    }
  }
  for (int64_t arena_bytes : {4 * dwords, 4 * dwords - 1, (int64_t)0}) {
    if (arena_bytes < 0) continue;
    uint8_t* arena = static_cast<uint8_t*>(malloc(arena_bytes ? arena_bytes : 1));
    memset(arena, 0xFF, arena_bytes ? arena_bytes : 1);
    compact_host(src, im, rep.end, bounds, dword.data(), 1, arena, arena_bytes);
    if (arena_bytes && memcmp(arena, want.data(), arena_bytes) != 0) die("arena differs from the serial pass", name);
    free(arena);
  }
  ++g_runs;
  g_no_end += rep.end == kNone;
  g_more += rep.n_rst > slots;
  g_fewer += rep.n_rst < slots;
  g_fill += rep.fill;
  free(bounds);
  free(src);
}

void sweep(const std::string& name, const std::vector<uint8_t>& bytes, int seg_cap) {
  run(name, bytes, seg_cap);
  Image probe{0, (int64_t)bytes.size(), 0, 1, 0, 0, 0};
  Report rep;
  scan_host(bytes.data(), probe, &rep, nullptr);                  // seg_cap 1: no slot is touched
  const int need = rep.n_rst + 1;
  for (int cap : {1, need - 1, need, need + 1})
    if (cap >= 1 && cap != seg_cap) run(name, bytes, cap);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s DIR   (of python tests/jpeg_scan_ref.py --dump DIR)\n", argv[0]);
    return 2;
  }
  DIR* dir = opendir(argv[1]);
  if (!dir) {
    perror(argv[1]);
    return 2;
  }
  int files = 0;
  while (dirent* e = readdir(dir)) {
    const std::string name = e->d_name;
    if (name.size() < 6 || name.substr(name.size() - 5) != ".scan") continue;
    const size_t dot = name.rfind('.', name.size() - 6);
    if (dot == std::string::npos) continue;
    const int seg_cap = atoi(name.c_str() + dot + 1);
    FILE* f = fopen((std::string(argv[1]) + "/" + name).c_str(), "rb");
    if (!f || seg_cap < 1) continue;
    std::vector<uint8_t> bytes;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);
    ++files;
    sweep(name, bytes, seg_cap);
  }
  closedir(dir);
  const long long from_files = g_runs;
  static const uint8_t alphabet[] = {0x00, 0x00, 0xFF, 0xFF, 0xFF, 0xD0, 0xD3, 0xD7, 0xD8, 0xCF, 0x41, 0x41, 0x7E, 0x7E, 0x01, 0x01};
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&state]() {                                        // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return state * 0x2545F4914F6CDD1Dull;
  };
  for (int i = 0; i < 20000; ++i) {
    const size_t n = i < 300 ? (size_t)(i % 20) : (size_t)(next() % 200);
    const bool rich = i % 4 == 0;                                   // markers anywhere, or only data, stuffing and restarts before a late end
    std::vector<uint8_t> bytes(n);
    for (auto& b : bytes) {
      b = alphabet[next() % sizeof alphabet];
      if (!rich && (b == 0xD8 || b == 0xCF)) b = 0xD1;
    }
    sweep("random " + std::to_string(i), bytes, 1 + (int)(next() % 6));
  }
  printf("%d corpus regions (%lld scans), %lld scans of random strings, %lld in all\n", files, from_files, g_runs - from_files, g_runs);
  printf("  no end: %lld, fill bytes: %lld, more restart markers than slots: %lld, fewer: %lld\n", g_no_end, g_fill, g_more, g_fewer);
  return files && g_more && g_fewer ? 0 : 1;
}
