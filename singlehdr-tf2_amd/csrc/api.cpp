// libshdr: error state and version (host only).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "shdr_internal.h"
#include "jpeg_enc.h"

namespace shdr {
static thread_local char g_last_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
}
}  // namespace shdr

namespace shdr {
int g_env_epoch = 0;
int64_t g_order_dependent_launches = 0;
}
extern "C" int64_t shdr_order_dependent_launches(void) {
  return __atomic_load_n(&shdr::g_order_dependent_launches, __ATOMIC_RELAXED);
}
extern "C" void shdr_config_reload(void) { __atomic_add_fetch(&shdr::g_env_epoch, 1, __ATOMIC_ACQ_REL); }

extern "C" const char* shdr_last_error(void) { return shdr::g_last_error; }
extern "C" const char* shdr_version(void) { return "libshdr 0.1 gfx950"; }

// CRC-32C (Castagnoli, reflected polynomial 0x82F63B78), slicing-by-8: the checksum of TensorFlow's tensor-bundle
// checkpoint format (.index blocks and tensor payloads; tf_utils.py:149-169 writes such checkpoints).  Host only.
namespace {
struct Crc32cTable {
  uint32_t t[8][256];
  Crc32cTable() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int s = 1; s < 8; ++s) t[s][i] = (t[s - 1][i] >> 8) ^ t[0][t[s - 1][i] & 0xff];
  }
};
}  // namespace

extern "C" uint32_t shdr_crc32c(const void* data, uint64_t n, uint32_t crc) {
  static const Crc32cTable tab;
  const unsigned char* p = static_cast<const unsigned char*>(data);
  uint32_t c = ~crc;
  while (n >= 8) {
    const uint32_t lo = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    c = tab.t[7][lo & 0xff] ^ tab.t[6][(lo >> 8) & 0xff] ^ tab.t[5][(lo >> 16) & 0xff] ^ tab.t[4][lo >> 24] ^
        tab.t[3][p[4]] ^ tab.t[2][p[5]] ^ tab.t[1][p[6]] ^ tab.t[0][p[7]];
    p += 8;
    n -= 8;
  }
  while (n--) c = tab.t[0][(c ^ *p++) & 0xff] ^ (c >> 8);
  return ~c;
}

// Radiance .hdr scanline run-length encoding ("new" adaptive RLE, each of the 4 RGBE components of a scanline coded
// separately: a count byte > 128 repeats the next byte (count - 128) times, a count <= 128 copies that many literal
// bytes).  This is the on-disk form cv2.imwrite("*.hdr") produces (test_real_refinement.py:150).  Host only.
namespace {
int64_t rle_component(const uint8_t* data, int n, uint8_t* out) {   // data stride 4 (one RGBE component)
  constexpr int kMinRun = 4;
  int64_t w = 0;
  int cur = 0;
  while (cur < n) {
    int run_start = cur, run_len = 0, prev_len = 0;
    while (run_len < kMinRun && run_start < n) {       // find the next run of at least kMinRun equal bytes
      run_start += run_len;
      prev_len = run_len;
      run_len = 1;
      while (run_start + run_len < n && run_len < 127 && data[4 * run_start] == data[4 * (run_start + run_len)]) ++run_len;
    }
    if (prev_len > 1 && prev_len == run_start - cur) {   // the bytes before it are themselves one short run
      out[w++] = (uint8_t)(128 + prev_len);
      out[w++] = data[4 * cur];
      cur = run_start;
    }
    while (cur < run_start) {                            // literals up to the run
      int lit = run_start - cur;
      if (lit > 128) lit = 128;
      out[w++] = (uint8_t)lit;
      for (int i = 0; i < lit; ++i) out[w++] = data[4 * (cur + i)];
      cur += lit;
    }
    if (run_len >= kMinRun) {
      out[w++] = (uint8_t)(128 + run_len);
      out[w++] = data[4 * run_start];
      cur += run_len;
    }
  }
  return w;
}
}  // namespace

extern "C" int64_t shdr_rgbe_rle_encode(const uint8_t* rgbe, int width, int height, uint8_t* out, int64_t capacity) {
  if (!rgbe || !out || width <= 0 || height <= 0) {
    shdr::set_error("rgbe_rle_encode: bad arguments");
    return -1;
  }
  const bool rle = width >= 8 && width <= 32767;         // outside this range the format stores flat pixels
  const int64_t per_line = rle ? 4 + 4 * ((int64_t)width + width / 127 + 2) : 4 * (int64_t)width;
  if (capacity < per_line * height) {
    shdr::set_error("rgbe_rle_encode: output buffer too small (%lld < %lld)", (long long)capacity, (long long)(per_line * height));
    return -1;
  }
  int64_t w = 0;
  for (int y = 0; y < height; ++y) {
    const uint8_t* line = rgbe + (int64_t)y * width * 4;
    if (!rle) {
      for (int64_t i = 0; i < 4 * (int64_t)width; ++i) out[w++] = line[i];
      continue;
    }
    out[w++] = 2; out[w++] = 2; out[w++] = (uint8_t)(width >> 8); out[w++] = (uint8_t)(width & 255);
    for (int c = 0; c < 4; ++c) w += rle_component(line + c, width, out + w);
  }
  return w;
}

// The inverse: every scanline is either flat (4 * width bytes) or, when 8 <= width <= 32767 and it starts with 2, 2 and
// the width, four run-length coded components -- the rule cv2.imread("*.hdr") applies (dataset.py:182).  Every read is
// checked against `size`, every write against the scanline.  Host only.
extern "C" int64_t shdr_rgbe_rle_decode(const uint8_t* data, int64_t size, int width, int height, uint8_t* rgbe) {
  if (!data || !rgbe || size < 0 || width <= 0 || height <= 0) {
    shdr::set_error("rgbe_rle_decode: bad arguments");
    return -1;
  }
  const bool rle_ok = width >= 8 && width <= 32767;
  int64_t pos = 0;
  for (int y = 0; y < height; ++y) {
    uint8_t* line = rgbe + (int64_t)y * width * 4;
    if (rle_ok && size - pos >= 4 && data[pos] == 2 && data[pos + 1] == 2 && ((int)data[pos + 2] << 8 | data[pos + 3]) == width) {
      pos += 4;
      for (int c = 0; c < 4; ++c) {
        int x = 0;
        while (x < width) {
          if (pos >= size) {
            shdr::set_error("rgbe_rle_decode: truncated data in scanline %d", y);
            return -1;
          }
          const int n = data[pos];
          if (n > 128) {                                    // a run of n - 128 copies of the next byte
            const int run = n - 128;
            if (pos + 1 >= size || x + run > width) {
              shdr::set_error("rgbe_rle_decode: %s in scanline %d", pos + 1 >= size ? "truncated data" : "corrupt run", y);
              return -1;
            }
            for (int i = 0; i < run; ++i) line[4 * (x + i) + c] = data[pos + 1];
            x += run;
            pos += 2;
          } else {                                          // n literal bytes
            if (pos + 1 + n > size || x + n > width) {
              shdr::set_error("rgbe_rle_decode: %s in scanline %d", pos + 1 + n > size ? "truncated data" : "corrupt literal", y);
              return -1;
            }
            for (int i = 0; i < n; ++i) line[4 * (x + i) + c] = data[pos + 1 + i];
            x += n;
            pos += 1 + n;
          }
        }
      }
    } else {
      if (size - pos < 4 * (int64_t)width) {
        shdr::set_error("rgbe_rle_decode: truncated data in flat scanline %d", y);
        return -1;
      }
      for (int64_t i = 0; i < 4 * (int64_t)width; ++i) line[i] = data[pos + i];
      pos += 4 * (int64_t)width;
    }
  }
  return pos;
}

// OpenEXR's RLE (exr.py): a signed count byte c; c < 0 -> -c literal bytes follow, otherwise the next byte repeated c + 1
// times.  Every read is checked against `size`, every write against `capacity`.  Host only.
extern "C" int64_t shdr_exr_rle_decode(const uint8_t* data, int64_t size, uint8_t* out, int64_t capacity) {
  if (!data || !out || size < 0 || capacity < 0) {
    shdr::set_error("exr_rle_decode: bad arguments");
    return -1;
  }
  int64_t pos = 0, w = 0;
  while (pos < size) {
    const int c = (int8_t)data[pos++];
    if (c < 0) {                                          // -c literal bytes
      const int64_t n = -c;
      if (n > size - pos || n > capacity - w) {
        shdr::set_error("exr_rle_decode: literal of %lld bytes at input byte %lld overruns the %s", (long long)n,
                        (long long)pos - 1, n > size - pos ? "input" : "output");
        return -1;
      }
      memcpy(out + w, data + pos, (size_t)n);
      pos += n;
      w += n;
    } else {                                              // a run of c + 1 copies of the next byte
      const int64_t n = (int64_t)c + 1;
      if (pos >= size || n > capacity - w) {
        shdr::set_error("exr_rle_decode: run of %lld bytes at input byte %lld overruns the %s", (long long)n, (long long)pos - 1,
                        pos >= size ? "input" : "output");
        return -1;
      }
      memset(out + w, data[pos], (size_t)n);
      pos += 1;
      w += n;
    }
  }
  return w;
}

// ---------------------------------------------------------------- baseline-JPEG writer: the host twin of csrc/jpeg_enc.hip
// The rules are csrc/jpeg_enc.h, shared with the kernels; these entries add the argument checks and the messages.  Host only.
namespace {
int enc_image(const char* what, const shdr_jpeg_enc_image* im, jpegenc::Image* out) {
  SHDR_REQUIRE(im, SHDR_E_NULL, "%s: null image descriptor", what);
  static_assert(sizeof(shdr_jpeg_enc_image) == sizeof(jpegenc::Image), "shdr_jpeg_enc_image and jpegenc::Image differ");
  memcpy(out, im, sizeof(*out));
  SHDR_REQUIRE(jpegenc::image_ok(*out), SHDR_E_SHAPE,
               "%s: need H and W in 1 .. 65535, layout 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), quality 1 .. 100 and a restart interval 0 .. "
               "65535, got %d x %d, layout %d, quality %d, restart %d", what, out->height, out->width, out->layout, out->quality, out->restart);
  return SHDR_OK;
}
int64_t enc_result(const char* what, int64_t n, int64_t bad_block, int64_t capacity) {
  if (n == jpegenc::kRangeError)
    return shdr::fail(SHDR_E_SHAPE, "%s: block %lld holds a coefficient outside the baseline range (an AC of category > 10 or a DC "
                      "difference of category > 11)", what, (long long)bad_block);
  if (n == jpegenc::kCapacityError) return shdr::fail(SHDR_E_SHAPE, "%s: the output does not fit into %lld bytes", what, (long long)capacity);
  return n;
}
}  // namespace

extern "C" int64_t shdr_jpeg_encode_blocks(const shdr_jpeg_enc_image* image, int64_t* out_bytes) {
  jpegenc::Image im;
  if (int rc = enc_image("jpeg_encode_blocks", image, &im)) return rc;
  const jpegenc::Geometry g = jpegenc::geometry(im);
  if (out_bytes) *out_bytes = jpegenc::out_bound(g);
  return g.blocks;
}

extern "C" int shdr_jpeg_encode_header_host(const shdr_jpeg_enc_image* image, uint8_t* out) {
  jpegenc::Image im;
  if (int rc = enc_image("jpeg_encode_header_host", image, &im)) return rc;
  SHDR_REQUIRE(out, SHDR_E_NULL, "jpeg_encode_header_host: null output");
  return jpegenc::compose_header(im, out);
}

extern "C" int64_t shdr_jpeg_encode_transform_host(const uint8_t* rgb, const shdr_jpeg_enc_image* image, int16_t* coef, int64_t coef_blocks) {
  const char* what = "jpeg_encode_transform_host";
  jpegenc::Image im;
  if (int rc = enc_image(what, image, &im)) return rc;
  SHDR_REQUIRE(rgb && coef, SHDR_E_NULL, "%s: null pointer", what);
  const jpegenc::Geometry g = jpegenc::geometry(im);
  SHDR_REQUIRE(coef_blocks >= g.blocks, SHDR_E_SHAPE, "%s: the arena holds %lld blocks, the image has %lld", what, (long long)coef_blocks,
               (long long)g.blocks);
  jpegenc::transform_host(rgb, im, coef);
  return g.blocks;
}

extern "C" int64_t shdr_jpeg_encode_entropy_host(const int16_t* coef, int64_t coef_blocks, const shdr_jpeg_enc_image* image, uint8_t* out,
                                                 int64_t capacity) {
  const char* what = "jpeg_encode_entropy_host";
  jpegenc::Image im;
  if (int rc = enc_image(what, image, &im)) return rc;
  SHDR_REQUIRE(coef && out, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(capacity >= 0, SHDR_E_SHAPE, "%s: negative capacity", what);
  const jpegenc::Geometry g = jpegenc::geometry(im);
  SHDR_REQUIRE(coef_blocks == g.blocks, SHDR_E_SHAPE, "%s: the arena holds %lld blocks, the image has %lld", what, (long long)coef_blocks,
               (long long)g.blocks);
  int64_t bad = -1;
  return enc_result(what, jpegenc::entropy_host(coef, im, out, capacity, &bad), bad, capacity);
}

extern "C" int64_t shdr_jpeg_encode_host(const uint8_t* rgb, const shdr_jpeg_enc_image* image, uint8_t* out, int64_t capacity) {
  const char* what = "jpeg_encode_host";
  jpegenc::Image im;
  if (int rc = enc_image(what, image, &im)) return rc;
  SHDR_REQUIRE(rgb && out, SHDR_E_NULL, "%s: null pointer", what);
  SHDR_REQUIRE(capacity >= 0, SHDR_E_SHAPE, "%s: negative capacity", what);
  const jpegenc::Geometry g = jpegenc::geometry(im);
  int16_t* coef = static_cast<int16_t*>(malloc((size_t)g.blocks * 128));
  SHDR_REQUIRE(coef, SHDR_E_SHAPE, "%s: no memory for %lld blocks", what, (long long)g.blocks);
  int64_t bad = -1;
  const int64_t n = jpegenc::encode_host(rgb, im, coef, out, capacity, &bad);
  free(coef);
  return enc_result(what, n, bad, capacity);
}
