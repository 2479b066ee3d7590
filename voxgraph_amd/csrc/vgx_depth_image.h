// What the depth-image decode (vgx_scan.hip) and the projective integrator (vgx_projective.hip) share: how a pixel's depth
// and colour are read (include/voxgraph_amd.h, "Depth-image scans": the depth and colour rules), and the check of a
// frame's layout, camera and byte counts.  gfx950 only.
#ifndef VGX_DEPTH_IMAGE_H_
#define VGX_DEPTH_IMAGE_H_

#include <cstdint>
#include <string>

#include "vgx_internal.h"

namespace vgx {

// the little-endian 32-bit field at p
template <bool DWORDS>
__device__ __forceinline__ uint32_t scan_field(const uint8_t* p) {
  if (DWORDS) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct DepthImage {
  const uint8_t* depth;
  const uint8_t* color;         // the colour image's base; not read for VGX_IMAGE_COLOR_NONE
  uint32_t n, wc;               // candidates; candidates per row of them
  unsigned long long wc_magic;  // ceil(2^64 / wc) for wc >= 2: i / wc == mulhi(i, wc_magic) for every i < 2^32 (wc < 2^31)
  uint32_t row_step, color_row_step, stride_u, stride_v;
  int32_t color_kind;
  float unit, min_z, max_z, cxf, cyf, kx, ky;
  uint32_t constant;              // constant_rgba as the word the colour array holds
  unsigned long long* counters;   // d_ctl + kScanDepthInvalid: running sums {invalid, out of range, overflowed}
};

// z of pixel u of the row at `row`: ELEMENTS loads the element, else its little-endian bytes one by one
template <int ENC, bool ELEMENTS>
__device__ __forceinline__ float depth_z(const DepthImage& m, const uint8_t* row, uint32_t u) {
  if (ENC == VGX_DEPTH_16UC1) {
    const uint8_t* p = row + 2 * (size_t)u;
    const uint32_t raw = ELEMENTS ? (uint32_t)*reinterpret_cast<const uint16_t*>(p) : ((uint32_t)p[0] | ((uint32_t)p[1] << 8));
    return (float)raw * m.unit;
  }
  return __uint_as_float(scan_field<ELEMENTS>(row + 4 * (size_t)u));
}

// the colour word (bytes r g b a, r lowest) of pixel (u, v) of the colour image; its pixels are read byte by byte (three
// bytes a pixel have no alignment to speak of)
__device__ __forceinline__ uint32_t depth_colour(const DepthImage& m, uint32_t u, uint32_t v) {
  const int32_t kind = m.color_kind;
  const uint32_t bpp = kind == VGX_IMAGE_COLOR_MONO8 ? 1u : ((kind == VGX_IMAGE_COLOR_RGB8 || kind == VGX_IMAGE_COLOR_BGR8) ? 3u : 4u);
  const uint8_t* p = m.color + (size_t)v * m.color_row_step + (size_t)u * bpp;
  const uint32_t b0 = p[0];
  if (bpp == 1u) return b0 | (b0 << 8) | (b0 << 16) | 0xff000000u;
  const uint32_t b1 = p[1], b2 = p[2], a = bpp == 4u ? (uint32_t)p[3] : 255u;
  const bool bgr = kind == VGX_IMAGE_COLOR_BGR8 || kind == VGX_IMAGE_COLOR_BGRA8;
  return (bgr ? b2 : b0) | (b1 << 8) | ((bgr ? b0 : b2) << 16) | (a << 24);
}

inline uint32_t depth_bpp(int32_t encoding) { return encoding == VGX_DEPTH_16UC1 ? 2u : 4u; }
inline uint32_t colour_bpp(int32_t kind) {
  return kind == VGX_IMAGE_COLOR_NONE ? 0u : (kind == VGX_IMAGE_COLOR_MONO8 ? 1u : (kind == VGX_IMAGE_COLOR_RGB8 || kind == VGX_IMAGE_COLOR_BGR8 ? 3u : 4u));
}

// vgx_depth_image_check with the reason (vgx_scan.hip)
int depth_image_check(const vgx_depth_image_layout* l, const vgx_depth_camera* cam, int64_t depth_n_bytes, int64_t color_n_bytes,
                      std::string* why);

}  // namespace vgx

#endif  // VGX_DEPTH_IMAGE_H_
