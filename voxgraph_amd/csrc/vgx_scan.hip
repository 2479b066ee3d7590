// A raw sensor_msgs/PointCloud2 decoded on the device: what PointcloudIntegrator::integratePointcloud does on the host
// before it reaches the integrator (pointcloud_integrator.cpp:29-63) -- pcl::fromROSMsg + voxblox::convertPointcloud
// [recalled]: drop the points that are not finite, one colour per kept point, message order kept.  The rules are stated
// in include/voxgraph_amd.h (vgx_scan), the measurement in DESIGN.md 17.
//
// ONE kernel whatever the size: a workgroup takes a tile of 1024 consecutive points (a ticket: TileChain,
// vgx_tsdf_internal.h), every thread reads four consecutive points and tests them, the kept ones are ranked inside the
// workgroup (block_exclusive_sum) and across the tiles before it (chain_exclusive_sum: the prefix sum inside the launch),
// and each thread writes its kept points and their colours at its rank.  No atomics decide a position: the order is the
// message's.  The last tile leaves the total for the host.
//
// The undistorting decode (include/voxgraph_amd.h, "Scan undistortion") is the same tile with one more step
// between the test and the ranking: the point's time field picks a segment of a pose track (a binary search over the
// knot times in global memory) and the point is moved into the reference frame by a linear blend of the two knots'
// transforms of it.  Three counters (bad time, overflowed, clamped) are summed per wave and added to running device
// words that are never cleared: the host subtracts what it read back last.
//
// The depth-image decode (include/voxgraph_amd.h, "Depth-image scans") fills the same handle from a
// sensor_msgs/Image and a pinhole model: depth_decode_tile below, with three more running counters of the same kind.
#include <cmath>
#include <cstring>
#include <string>

#include "vgx_internal.h"
#include "vgx_tsdf_internal.h"
#include "vgx_depth_image.h"

#pragma clang fp contract(off)

namespace vgx {

constexpr int kScanIpt = 4;                    // consecutive points per thread
constexpr int kScanTile = 256 * kScanIpt;      // points per workgroup
constexpr size_t kScanStageBytes = 1u << 20;   // one pinned staging buffer (two of them, filled in turn)
// (the u64 words of vgx_scan_s::d_ctl, kScan*, and vgx_scan_s itself: vgx_tsdf_internal.h)

struct ScanMsg {
  const uint8_t* data;
  uint32_t n, width, point_step, row_step;
  uint32_t offset_x, offset_y, offset_z, color_offset;
  int32_t color_kind;
  float intensity_min, intensity_max;
  uint32_t constant;  // constant_rgba as the word the colour array holds (r in the low byte)
};

// the undistorting decode's arguments: the time field and the track (device copies of the caller's arrays)
struct ScanDeskew {
  const double* knot_time;  // [n_knots] strictly ascending
  const float* knot_T;      // [n_knots][7] qw qx qy qz tx ty tz: T_ref_sensor(knot_time[k])
  int32_t n_knots, time_kind;
  uint32_t time_offset;
  double scale, offset_s;
  unsigned long long* counters;  // d_ctl + kScanBadTime: running sums {bad time, overflowed, clamped}
};

__device__ __forceinline__ bool scan_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// the colour word (bytes r g b a, r lowest) of a kept point from the 4 bytes at its colour field
__device__ __forceinline__ uint32_t scan_colour(const ScanMsg& m, uint32_t field) {
  if (m.color_kind == VGX_SCAN_COLOR_RGB)  // b0 b1 b2 b3 -> (b2, b1, b0, b3)
    return ((field >> 16) & 0xffu) | (field & 0xff00u) | ((field & 0xffu) << 16) | (field & 0xff000000u);
  float v = __uint_as_float(field);
  v = (m.intensity_min < v) ? v : m.intensity_min;  // std::max(min, v): NaN -> min
  v = (v < m.intensity_max) ? v : m.intensity_max;  // std::min(max, v)
  const float h = (v - m.intensity_min) / (m.intensity_max - m.intensity_min);
  const uint32_t g = (uint32_t)(uint8_t)round((double)h * 255.0);
  return g | (g << 8) | (g << 16) | 0xff000000u;
}

// t = offset_s + (double)raw * scale of the point at p: one rounded f64 multiply, one rounded f64 add
template <bool DWORDS>
__device__ __forceinline__ double scan_time(const ScanDeskew& u, const uint8_t* p) {
  const uint32_t lo = scan_field<DWORDS>(p + u.time_offset);
  double raw;
  if (u.time_kind == VGX_SCAN_TIME_UINT32)
    raw = (double)lo;
  else if (u.time_kind == VGX_SCAN_TIME_FLOAT32)
    raw = (double)__uint_as_float(lo);
  else  // (an 8-byte field as two words: it need not be 8-aligned)
    raw = __longlong_as_double((long long)(((unsigned long long)scan_field<DWORDS>(p + u.time_offset + 4) << 32) | lo));
  const double scaled = raw * u.scale;
  return u.offset_s + scaled;
}

// The point (x, y, z) observed at the finite time t, in the reference frame: the segment k = (knots with time <= t) - 1,
// a in [0, 1] inside it (the f32 of a ratio below 1 may be 1), g0 + a * (g1 - g0) of the two knots' transforms of the point.  Before the first knot and from
// the last knot on a = 0: the knot's transform alone.  clamped: t lies outside the track.
__device__ __forceinline__ void scan_undistort(const ScanDeskew& u, double t, float& x, float& y, float& z, bool& clamped) {
  int lo = 0, hi = u.n_knots;  // the number of knots with time <= t lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (u.knot_time[mid] <= t)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int k = lo > 0 ? lo - 1 : 0;
  float a = 0.0f;
  clamped = lo == 0;
  if (lo == u.n_knots) {
    clamped = t > u.knot_time[k];
  } else if (lo > 0) {
    const double t0 = u.knot_time[k], t1 = u.knot_time[k + 1];
    a = (float)((t - t0) / (t1 - t0));
  }
  const float* T = u.knot_T + 7 * (size_t)k;
  float g0x, g0y, g0z;
  transform_point(T[0], T[1], T[2], T[3], T[4], T[5], T[6], x, y, z, g0x, g0y, g0z);
  if (a != 0.0f) {
    float g1x, g1y, g1z;
    transform_point(T[7], T[8], T[9], T[10], T[11], T[12], T[13], x, y, z, g1x, g1y, g1z);
    g0x = g0x + a * (g1x - g0x);
    g0y = g0y + a * (g1y - g0y);
    g0z = g0z + a * (g1z - g0z);
  }
  x = g0x;
  y = g0y;
  z = g0z;
}

// one tile of a decode; u == nullptr unless DESKEW
template <bool DWORDS, bool DESKEW>
__device__ __forceinline__ void scan_decode_tile(const ScanMsg& m, const ScanDeskew* u, const TileChain& chain,
                                                 float* __restrict__ points, uint32_t* __restrict__ rgba,
                                                 unsigned long long* __restrict__ total) {
  __shared__ uint32_t sh_word, sh4[4];
  const uint32_t tile = chain_tile(chain, &sh_word);
  const uint32_t base = (tile * 256u + threadIdx.x) * (uint32_t)kScanIpt;  // (n < 2^31: no overflow)
  uint32_t x[kScanIpt], y[kScanIpt], z[kScanIpt], c[kScanIpt], keep = 0;
  uint32_t counts = 0;  // DESKEW: this thread's bad times | overflowed << 10 | clamped << 20 (a wave's sum: 256 at most each)
#pragma unroll
  for (int e = 0; e < kScanIpt; ++e) {
    const uint32_t i = base + (uint32_t)e;
    x[e] = y[e] = z[e] = 0u;
    c[e] = m.constant;
    if (i < m.n) {
      const uint32_t row = i / m.width, col = i - row * m.width;
      const uint8_t* p = m.data + (size_t)row * m.row_step + (size_t)col * m.point_step;
      x[e] = scan_field<DWORDS>(p + m.offset_x);
      y[e] = scan_field<DWORDS>(p + m.offset_y);
      z[e] = scan_field<DWORDS>(p + m.offset_z);
      bool kept = scan_finite(x[e]) && scan_finite(y[e]) && scan_finite(z[e]);
      if (DESKEW && kept) {
        const double t = scan_time<DWORDS>(*u, p);
        if (!(fabs(t) < INFINITY)) {
          kept = false;
          counts += 1u;
        } else {
          float gx = __uint_as_float(x[e]), gy = __uint_as_float(y[e]), gz = __uint_as_float(z[e]);
          bool clamped;
          scan_undistort(*u, t, gx, gy, gz, clamped);
          x[e] = __float_as_uint(gx);
          y[e] = __float_as_uint(gy);
          z[e] = __float_as_uint(gz);
          kept = scan_finite(x[e]) && scan_finite(y[e]) && scan_finite(z[e]);
          counts += kept ? (clamped ? 1u << 20 : 0u) : 1u << 10;
        }
      }
      if (kept) {
        keep |= 1u << e;
        if (m.color_kind != VGX_SCAN_COLOR_NONE) c[e] = scan_colour(m, scan_field<DWORDS>(p + m.color_offset));
      }
    }
  }
  if (DESKEW) {
    for (int d = 32; d > 0; d >>= 1) counts += (uint32_t)__shfl_xor((int)counts, d);
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t v = (counts >> (10 * k)) & 0x3ffu;
        if (v) atomicAdd(u->counters + k, (unsigned long long)v);
      }
    }
  }
  uint32_t in_tile = 0;
  const uint32_t before = block_exclusive_sum((uint32_t)__popc(keep), sh4, in_tile);
  const uint32_t prefix = chain_exclusive_sum(chain, tile, in_tile, &sh_word);
  if (tile == gridDim.x - 1 && threadIdx.x == 0) *total = (unsigned long long)prefix + in_tile;
  size_t at = (size_t)prefix + before;
#pragma unroll
  for (int e = 0; e < kScanIpt; ++e) {
    if ((keep >> e) & 1u) {
      points[3 * at + 0] = __uint_as_float(x[e]);
      points[3 * at + 1] = __uint_as_float(y[e]);
      points[3 * at + 2] = __uint_as_float(z[e]);
      rgba[at] = c[e];
      ++at;
    }
  }
}

template <bool DWORDS>
__global__ __launch_bounds__(256) void scan_decode_kernel(ScanMsg m, TileChain chain, float* __restrict__ points,
                                                          uint32_t* __restrict__ rgba, unsigned long long* __restrict__ total) {
  scan_decode_tile<DWORDS, false>(m, nullptr, chain, points, rgba, total);
}

template <bool DWORDS>
__global__ __launch_bounds__(256) void scan_decode_undistort_kernel(ScanMsg m, ScanDeskew u, TileChain chain,
                                                                    float* __restrict__ points, uint32_t* __restrict__ rgba,
                                                                    unsigned long long* __restrict__ total) {
  scan_decode_tile<DWORDS, true>(m, &u, chain, points, rgba, total);
}

// ---- depth images (include/voxgraph_amd.h, "Depth-image scans") ------------------------------------------
// The same tile with a pinhole model in front of it: a candidate is a pixel the strides keep, its depth becomes z, the
// gate and the unprojection decide whether it is kept, and from there on (track step, ranking, stores) it is a point
// of scan_decode_tile.  A thread's four candidates are consecutive in the image's row-major order, so a wave reads 256
// consecutive pixels of (mostly) one row and writes its kept points side by side.
// one tile of a depth-image decode; u == nullptr unless DESKEW (of *u the track, scale, offset_s and counters are read)
template <int ENC, bool ELEMENTS, bool DESKEW>
__device__ __forceinline__ void depth_decode_tile(const DepthImage& m, const ScanDeskew* u, const TileChain& chain,
                                                  float* __restrict__ points, uint32_t* __restrict__ rgba,
                                                  unsigned long long* __restrict__ total) {
  __shared__ uint32_t sh_word, sh4[4];
  const uint32_t tile = chain_tile(chain, &sh_word);
  const uint32_t base = (tile * 256u + threadIdx.x) * (uint32_t)kScanIpt;  // (n < 2^31: no overflow)
  // the candidate row and column of the thread's first candidate (no division: the host's reciprocal), then stepped
  uint32_t rc = m.wc == 1u ? base : (uint32_t)__umul64hi((unsigned long long)base, m.wc_magic);
  uint32_t cc = base - rc * m.wc;
  uint32_t x[kScanIpt], y[kScanIpt], z[kScanIpt], c[kScanIpt], keep = 0;
  uint32_t dcounts = 0;  // this thread's invalid | out of range << 10 | overflowed << 20 (a wave's sum: 256 at most each)
  uint32_t counts = 0;   // DESKEW: bad times | overflowed << 10 | clamped << 20, as scan_decode_tile counts them
#pragma unroll
  for (int e = 0; e < kScanIpt; ++e) {
    x[e] = y[e] = z[e] = 0u;
    c[e] = m.constant;
    if (base + (uint32_t)e < m.n) {
      const uint32_t pu = cc * m.stride_u, pv = rc * m.stride_v;  // the pixel: inside the image, as rc < hc and cc < wc
      const float zf = depth_z<ENC, ELEMENTS>(m, m.depth + (size_t)pv * m.row_step, pu);
      if (!(0.0f < zf && zf < INFINITY)) {
        dcounts += 1u;
      } else if (!(m.min_z <= zf && zf <= m.max_z)) {
        dcounts += 1u << 10;
      } else {
        float gx = (((float)pu - m.cxf) * zf) * m.kx;
        float gy = (((float)pv - m.cyf) * zf) * m.ky;
        float gz = zf;
        bool kept = scan_finite(__float_as_uint(gx)) && scan_finite(__float_as_uint(gy));
        if (!kept) dcounts += 1u << 20;
        if (DESKEW && kept) {
          const double scaled = (double)pv * u->scale;
          const double t = u->offset_s + scaled;
          if (!(fabs(t) < INFINITY)) {
            kept = false;
            counts += 1u;
          } else {
            bool clamped;
            scan_undistort(*u, t, gx, gy, gz, clamped);
            kept = scan_finite(__float_as_uint(gx)) && scan_finite(__float_as_uint(gy)) && scan_finite(__float_as_uint(gz));
            counts += kept ? (clamped ? 1u << 20 : 0u) : 1u << 10;
          }
        }
        if (kept) {
          keep |= 1u << e;
          x[e] = __float_as_uint(gx);
          y[e] = __float_as_uint(gy);
          z[e] = __float_as_uint(gz);
          if (m.color_kind != VGX_IMAGE_COLOR_NONE) c[e] = depth_colour(m, pu, pv);
        }
      }
    }
    if (++cc == m.wc) {
      cc = 0;
      ++rc;
    }
  }
  // the counters: summed per wave, then per workgroup behind block_exclusive_sum's barriers, so that a tile adds to each
  // running word once (nearly every wave of a real frame meets an invalid pixel: an atomic a wave on one word is a queue)
  __shared__ uint32_t sh_counts[2][4];
  for (int d = 32; d > 0; d >>= 1) {
    dcounts += (uint32_t)__shfl_xor((int)dcounts, d);
    if (DESKEW) counts += (uint32_t)__shfl_xor((int)counts, d);
  }
  if ((threadIdx.x & 63u) == 0) {
    sh_counts[0][threadIdx.x >> 6] = dcounts;
    sh_counts[1][threadIdx.x >> 6] = counts;
  }
  uint32_t in_tile = 0;
  const uint32_t before = block_exclusive_sum((uint32_t)__popc(keep), sh4, in_tile);
  if (threadIdx.x < (DESKEW ? 6u : 3u)) {
    const uint32_t set = threadIdx.x / 3u, k = threadIdx.x - 3u * set;
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) v += (sh_counts[set][w] >> (10u * k)) & 0x3ffu;
    if (v) atomicAdd((set ? u->counters : m.counters) + k, (unsigned long long)v);
  }
  const uint32_t prefix = chain_exclusive_sum(chain, tile, in_tile, &sh_word);
  if (tile == gridDim.x - 1 && threadIdx.x == 0) *total = (unsigned long long)prefix + in_tile;
  size_t at = (size_t)prefix + before;
#pragma unroll
  for (int e = 0; e < kScanIpt; ++e) {
    if ((keep >> e) & 1u) {
      points[3 * at + 0] = __uint_as_float(x[e]);
      points[3 * at + 1] = __uint_as_float(y[e]);
      points[3 * at + 2] = __uint_as_float(z[e]);
      rgba[at] = c[e];
      ++at;
    }
  }
}

template <int ENC, bool ELEMENTS>
__global__ __launch_bounds__(256) void depth_decode_kernel(DepthImage m, TileChain chain, float* __restrict__ points,
                                                           uint32_t* __restrict__ rgba, unsigned long long* __restrict__ total) {
  depth_decode_tile<ENC, ELEMENTS, false>(m, nullptr, chain, points, rgba, total);
}

template <int ENC, bool ELEMENTS>
__global__ __launch_bounds__(256) void depth_decode_undistort_kernel(DepthImage m, ScanDeskew u, TileChain chain,
                                                                     float* __restrict__ points, uint32_t* __restrict__ rgba,
                                                                     unsigned long long* __restrict__ total) {
  depth_decode_tile<ENC, ELEMENTS, true>(m, &u, chain, points, rgba, total);
}

}  // namespace vgx

using namespace vgx;

namespace vgx {
vgx_ctx scan_context(vgx_scan S) { return S ? S->ctx : nullptr; }
std::unique_lock<std::mutex> scan_borrow(vgx_scan S, const float** d_points, int64_t* n) {
  std::unique_lock<std::mutex> lk(S->mu);
  *n = S->n_points;
  *d_points = S->n_points > 0 ? S->d_points.as<float>() : nullptr;
  return lk;
}
std::unique_lock<std::mutex> scan_borrow(vgx_scan S, const float** d_points, const uint32_t** d_rgba, int64_t* n) {
  std::unique_lock<std::mutex> lk = scan_borrow(S, d_points, n);
  *d_rgba = S->n_points > 0 ? S->d_rgba.as<uint32_t>() : nullptr;
  return lk;
}
}  // namespace vgx

namespace {

// Everything a decode is refused for that the layout, the configuration and the byte count alone decide; VGX_OK, or the
// code with `why`.
int scan_check(const vgx_scan_layout* l, const vgx_scan_config* c, int64_t n_bytes, std::string* why) {
  auto fail = [why](int code, const char* msg) {
    if (why) *why = msg;
    return code;
  };
  if (!l) return fail(VGX_ERR_INVALID, "NULL layout");
  if (n_bytes < 0) return fail(VGX_ERR_INVALID, "n_bytes is negative");
  if (l->point_step == 0) return fail(VGX_ERR_INVALID, "point_step is 0");
  if (l->color_kind != VGX_SCAN_COLOR_NONE && l->color_kind != VGX_SCAN_COLOR_RGB && l->color_kind != VGX_SCAN_COLOR_INTENSITY)
    return fail(VGX_ERR_INVALID, "unknown color_kind");
  const uint64_t step = l->point_step;
  if ((uint64_t)l->offset_x + 4 > step || (uint64_t)l->offset_y + 4 > step || (uint64_t)l->offset_z + 4 > step)
    return fail(VGX_ERR_INVALID, "a coordinate field does not fit in point_step");
  if (l->color_kind != VGX_SCAN_COLOR_NONE && (uint64_t)l->color_offset + 4 > step)
    return fail(VGX_ERR_INVALID, "the colour field does not fit in point_step");
  if ((uint64_t)l->row_step < (uint64_t)l->width * step) return fail(VGX_ERR_INVALID, "row_step is less than width * point_step");
  if (c && (!std::isfinite(c->intensity_min) || !std::isfinite(c->intensity_max) || !(c->intensity_max > c->intensity_min)))
    return fail(VGX_ERR_INVALID, "the intensity range is not finite or not max > min");
  if (l->is_bigendian != 0) return fail(VGX_ERR_UNSUPPORTED, "big-endian messages are not supported");
  const uint64_t n = (uint64_t)l->width * l->height;
  if (n >= (1ull << 31)) return fail(VGX_ERR_UNSUPPORTED, "width * height is 2^31 or more");
  if (n > 0 && (uint64_t)n_bytes < (uint64_t)(l->height - 1) * l->row_step + (uint64_t)l->width * step)
    return fail(VGX_ERR_INVALID, "n_bytes is less than (height - 1) * row_step + width * point_step");
  return VGX_OK;
}

// what a track (not NULL) is refused for
int scan_track_check(const vgx_scan_track* tr, std::string* why) {
  auto fail = [why](const char* msg) {
    if (why) *why = msg;
    return (int)VGX_ERR_INVALID;
  };
  if (tr->n_knots < 1 || tr->n_knots > VGX_SCAN_TRACK_MAX_KNOTS) return fail("n_knots is not in 1 .. 65536");
  if (!tr->knot_time || !tr->knot_T) return fail("NULL knot array");
  for (int32_t k = 0; k < tr->n_knots; ++k) {
    if (!std::isfinite(tr->knot_time[k]) || (k > 0 && !(tr->knot_time[k] > tr->knot_time[k - 1])))
      return fail("the knot times are not finite and strictly ascending");
    for (int j = 0; j < 7; ++j)
      if (!std::isfinite(tr->knot_T[7 * (size_t)k + j])) return fail("a knot_T entry is not finite");
  }
  return VGX_OK;
}

// Everything an undistorting decode is refused for on top of scan_check.
int scan_undistort_check(const vgx_scan_layout* l, const vgx_scan_config* c, const vgx_scan_time_field* f, const vgx_scan_track* tr,
                         int64_t n_bytes, std::string* why) {
  auto fail = [why](const char* msg) {
    if (why) *why = msg;
    return (int)VGX_ERR_INVALID;
  };
  if (!f) return fail("NULL time field");
  if (!tr) return fail("NULL track");
  const int rc = scan_check(l, c, n_bytes, why);
  if (rc != VGX_OK) return rc;
  if (f->kind != VGX_SCAN_TIME_UINT32 && f->kind != VGX_SCAN_TIME_FLOAT32 && f->kind != VGX_SCAN_TIME_FLOAT64)
    return fail("unknown time kind");
  if ((uint64_t)f->offset + (f->kind == VGX_SCAN_TIME_FLOAT64 ? 8u : 4u) > (uint64_t)l->point_step)
    return fail("the time field does not fit in point_step");
  if (!std::isfinite(f->scale) || !std::isfinite(f->offset_s)) return fail("the time field's scale or offset_s is not finite");
  return scan_track_check(tr, why);
}

// Everything a depth-image decode is refused for that the layout, the camera, the configuration and the byte counts alone
// decide.
int depth_check(const vgx_depth_image_layout* l, const vgx_depth_camera* cam, const vgx_scan_config* c, int64_t depth_n_bytes,
                int64_t color_n_bytes, std::string* why) {
  auto fail = [why](int code, const char* msg) {
    if (why) *why = msg;
    return code;
  };
  if (!l) return fail(VGX_ERR_INVALID, "NULL layout");
  if (!cam) return fail(VGX_ERR_INVALID, "NULL camera");
  if (l->encoding != VGX_DEPTH_16UC1 && l->encoding != VGX_DEPTH_32FC1) return fail(VGX_ERR_INVALID, "unknown depth encoding");
  if (l->color_kind < VGX_IMAGE_COLOR_NONE || l->color_kind > VGX_IMAGE_COLOR_MONO8) return fail(VGX_ERR_INVALID, "unknown color_kind");
  const bool colour = l->color_kind != VGX_IMAGE_COLOR_NONE;
  if (depth_n_bytes < 0 || (colour && color_n_bytes < 0)) return fail(VGX_ERR_INVALID, "n_bytes is negative");
  const uint64_t bpp = depth_bpp(l->encoding), cbpp = colour_bpp(l->color_kind);
  if ((uint64_t)l->row_step < (uint64_t)l->width * bpp) return fail(VGX_ERR_INVALID, "row_step is less than width * bytes per pixel");
  if (colour && (uint64_t)l->color_row_step < (uint64_t)l->width * cbpp)
    return fail(VGX_ERR_INVALID, "color_row_step is less than width * bytes per pixel");
  if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0 || cam->fy == 0.0)
    return fail(VGX_ERR_INVALID, "fx or fy is zero or not finite");
  if (!std::isfinite(cam->cx) || !std::isfinite(cam->cy)) return fail(VGX_ERR_INVALID, "cx or cy is not finite");
  if (l->encoding == VGX_DEPTH_16UC1 && (!std::isfinite(cam->depth_unit_m) || !(cam->depth_unit_m > 0.0f)))
    return fail(VGX_ERR_INVALID, "depth_unit_m is not finite or not positive");
  if (std::isnan(cam->min_depth_m) || std::isnan(cam->max_depth_m) || cam->min_depth_m < 0.0f || cam->min_depth_m > cam->max_depth_m)
    return fail(VGX_ERR_INVALID, "the depth bounds are NaN, negative or not min <= max");
  if (cam->stride_u < 1 || cam->stride_v < 1) return fail(VGX_ERR_INVALID, "a stride is less than 1");
  if (c && (!std::isfinite(c->intensity_min) || !std::isfinite(c->intensity_max) || !(c->intensity_max > c->intensity_min)))
    return fail(VGX_ERR_INVALID, "the intensity range is not finite or not max > min");
  if (l->is_bigendian != 0) return fail(VGX_ERR_UNSUPPORTED, "big-endian images are not supported");
  const uint64_t n = (uint64_t)l->width * l->height;
  if (n >= (1ull << 31)) return fail(VGX_ERR_UNSUPPORTED, "width * height is 2^31 or more");
  if (n > 0 && (uint64_t)depth_n_bytes < (uint64_t)(l->height - 1) * l->row_step + (uint64_t)l->width * bpp)
    return fail(VGX_ERR_INVALID, "depth_n_bytes is less than (height - 1) * row_step + width * bytes per pixel");
  if (n > 0 && colour && (uint64_t)color_n_bytes < (uint64_t)(l->height - 1) * l->color_row_step + (uint64_t)l->width * cbpp)
    return fail(VGX_ERR_INVALID, "color_n_bytes is less than (height - 1) * color_row_step + width * bytes per pixel");
  return VGX_OK;
}

// ... and an undistorting one on top of depth_check
int depth_undistort_check(const vgx_depth_image_layout* l, const vgx_depth_camera* cam, const vgx_scan_config* c,
                          const vgx_depth_row_time* rt, const vgx_scan_track* tr, int64_t depth_n_bytes, int64_t color_n_bytes,
                          std::string* why) {
  auto fail = [why](const char* msg) {
    if (why) *why = msg;
    return (int)VGX_ERR_INVALID;
  };
  if (!rt) return fail("NULL row time");
  if (!tr) return fail("NULL track");
  const int rc = depth_check(l, cam, c, depth_n_bytes, color_n_bytes, why);
  if (rc != VGX_OK) return rc;
  if (!std::isfinite(rt->scale) || !std::isfinite(rt->offset_s)) return fail("the row time's scale or offset_s is not finite");
  return scan_track_check(tr, why);
}

// the caller's bytes -> S->d_msg + dst on stream st.  Through the pinned buffers piece by piece: the host copy of piece k
// overlaps the upload of piece k - 1, and the caller's bytes have been read when the last piece is queued.
int scan_upload(vgx_scan S, hipStream_t st, const void* data, size_t bytes, size_t dst = 0) {
  vgx_ctx ctx = S->ctx;
  if (!S->pageable && S->stage.reserve(kScanStageBytes) != hipSuccess) {
    (void)hipGetLastError();  // no pinned memory to be had: remembered, the pageable path below from now on
    S->pageable = true;
  }
  if (S->pageable) {
    VGX_HIP(ctx, hipMemcpyAsync(S->d_msg.as<char>() + dst, data, bytes, hipMemcpyHostToDevice, st));
    return VGX_OK;  // (the decode's closing synchronisation is behind it: the bytes are the caller's again on return)
  }
  for (size_t at = 0; at < bytes; at += kScanStageBytes) {
    const size_t piece = std::min(kScanStageBytes, bytes - at);
    // (waits for this half's last upload: of this call, or of an earlier one that failed before its closing
    // synchronisation; an event never recorded is complete)
    int k = 0;
    hipError_t waited = hipSuccess;
    void* h = S->stage.next(&k, &waited);
    VGX_HIP(ctx, waited);
    std::memcpy(h, static_cast<const char*>(data) + at, piece);
    VGX_HIP(ctx, hipMemcpyAsync(S->d_msg.as<char>() + dst + at, h, piece, hipMemcpyHostToDevice, st));
    VGX_HIP(ctx, S->stage.record(k, st));
  }
  return VGX_OK;
}

// Room for a decode of n candidates in `tiles` tiles, queued on the TSDF stream: the arrays, the control words and the
// tile words.
int scan_reserve(vgx_scan S, uint32_t n, uint32_t tiles) {
  vgx_ctx ctx = S->ctx;
  hipStream_t st = ctx->tsdf_stream;
  if ((size_t)n * 4 > S->d_rgba.bytes) {
    VGX_HIP(ctx, hipStreamSynchronize(st));  // (a queued scan may still read the arrays)
    const hipError_t e = alloc_group({{&S->d_points, (size_t)n * 12}, {&S->d_rgba, (size_t)n * 4}});
    if (e != hipSuccess) return alloc_error(ctx, e, "scan: allocating points and colours");
  }
  if (!S->d_ctl.p) {
    const hipError_t e = S->d_ctl.alloc(kScanCtlWords * 8);
    if (e != hipSuccess) return alloc_error(ctx, e, "scan: allocating counters");
    VGX_HIP(ctx, hipMemsetAsync(S->d_ctl.p, 0, kScanCtlWords * 8, st));
    S->clock.tickets = 0;
  }
  if ((size_t)tiles * 8 > S->d_state.bytes) {
    VGX_HIP(ctx, hipStreamSynchronize(st));
    const hipError_t e = S->d_state.alloc((size_t)tiles * 8);
    if (e != hipSuccess) return alloc_error(ctx, e, "scan: allocating tile words");
    VGX_HIP(ctx, hipMemsetAsync(S->d_state.p, 0, S->d_state.bytes, st));  // (epoch 0: no launch's tag)
  }
  return VGX_OK;
}

// The launch's chain, after scan_reserve.  Right before the launch: nothing that can fail may come between.
int scan_chain(vgx_scan S, uint32_t tiles, TileChain* chain) {
  vgx_ctx ctx = S->ctx;
  ChainTake t;
  VGX_HIP(ctx, chain_take(&S->clock, tiles, S->d_state, ctx->tsdf_stream, &t));
  unsigned long long* ctl = S->d_ctl.as<unsigned long long>();
  chain->state = S->d_state.as<unsigned long long>();
  chain->epoch = t.epoch;
  chain->ticket = ctl + kScanTicket;
  chain->ticket_base = t.ticket_base;
  chain->error = ctl + kScanError;
  return VGX_OK;
}

// The running counters of d_ctl are about to be added to by a launch: cleared first where the last such launch's
// read-back failed, and not known again until this one's has come.
int scan_counters_open(vgx_scan S) {
  vgx_ctx ctx = S->ctx;
  if (!S->counters_known) {
    VGX_HIP(ctx, hipMemsetAsync(S->d_ctl.as<unsigned long long>() + kScanBadTime, 0, 48, ctx->tsdf_stream));
    for (int k = 0; k < 3; ++k) S->counters_base[k] = S->depth_base[k] = 0;
  }
  S->counters_known = false;
  return VGX_OK;
}

// the track goes up ahead of the launch: the times, then the transforms, in one buffer of the handle's
int scan_track_upload(vgx_scan S, const vgx_scan_track* tr, ScanDeskew* u) {
  vgx_ctx ctx = S->ctx;
  hipStream_t st = ctx->tsdf_stream;
  const size_t K = (size_t)tr->n_knots;
  if (K * 36 > S->d_knots.bytes) {
    VGX_HIP(ctx, hipStreamSynchronize(st));
    const hipError_t e = S->d_knots.alloc(K * 36);
    if (e != hipSuccess) return alloc_error(ctx, e, "scan: allocating the track");
  }
  VGX_HIP(ctx, hipMemcpyAsync(S->d_knots.p, tr->knot_time, K * 8, hipMemcpyHostToDevice, st));
  VGX_HIP(ctx, hipMemcpyAsync(S->d_knots.as<char>() + K * 8, tr->knot_T, K * 28, hipMemcpyHostToDevice, st));
  u->knot_time = S->d_knots.as<double>();
  u->knot_T = reinterpret_cast<const float*>(S->d_knots.as<char>() + K * 8);
  u->n_knots = tr->n_knots;
  u->counters = S->d_ctl.as<unsigned long long>() + kScanBadTime;
  return VGX_OK;
}

// The decode of a message at d_data (device) on the TSDF stream; the caller holds S->mu and ctx->tsdf_mu, the device is
// set, the layout (and f, tr where given: the undistorting decode) has passed its check.  Ends with the call's one host
// synchronisation.
int scan_decode_queued(vgx_scan S, const vgx_scan_layout& l, const vgx_scan_config& c, const vgx_scan_time_field* f,
                       const vgx_scan_track* tr, const uint8_t* d_data) {
  vgx_ctx ctx = S->ctx;
  hipStream_t st = ctx->tsdf_stream;
  const uint32_t n = l.width * l.height;
  const uint32_t tiles = (n + kScanTile - 1) / kScanTile;
  int rc = scan_reserve(S, n, tiles);
  if (rc != VGX_OK) return rc;
  unsigned long long* ctl = S->d_ctl.as<unsigned long long>();
  ScanMsg m{};
  m.data = d_data;
  m.n = n;
  m.width = l.width;
  m.point_step = l.point_step;
  m.row_step = l.row_step;
  m.offset_x = l.offset_x;
  m.offset_y = l.offset_y;
  m.offset_z = l.offset_z;
  m.color_offset = l.color_kind == VGX_SCAN_COLOR_NONE ? 0u : l.color_offset;
  m.color_kind = l.color_kind;
  m.intensity_min = c.intensity_min;
  m.intensity_max = c.intensity_max;
  std::memcpy(&m.constant, c.constant_rgba, 4);
  bool dwords = ((uintptr_t)d_data | l.point_step | l.row_step | l.offset_x | l.offset_y | l.offset_z | m.color_offset) % 4 == 0;
  // (the chain is taken right before the launch: nothing that can fail may come between)
  TileChain chain;
  if (!tr) {
    if ((rc = scan_chain(S, tiles, &chain)) != VGX_OK) return rc;
    if (dwords)
      hipLaunchKernelGGL(scan_decode_kernel<true>, dim3(tiles), dim3(256), 0, st, m, chain, S->d_points.as<float>(),
                         S->d_rgba.as<uint32_t>(), ctl + kScanTotal);
    else
      hipLaunchKernelGGL(scan_decode_kernel<false>, dim3(tiles), dim3(256), 0, st, m, chain, S->d_points.as<float>(),
                         S->d_rgba.as<uint32_t>(), ctl + kScanTotal);
  } else {
    ScanDeskew u{};
    if ((rc = scan_track_upload(S, tr, &u)) != VGX_OK || (rc = scan_counters_open(S)) != VGX_OK) return rc;
    u.time_kind = f->kind;
    u.time_offset = f->offset;
    u.scale = f->scale;
    u.offset_s = f->offset_s;
    dwords = dwords && f->offset % 4 == 0;
    if ((rc = scan_chain(S, tiles, &chain)) != VGX_OK) return rc;
    if (dwords)
      hipLaunchKernelGGL(scan_decode_undistort_kernel<true>, dim3(tiles), dim3(256), 0, st, m, u, chain, S->d_points.as<float>(),
                         S->d_rgba.as<uint32_t>(), ctl + kScanTotal);
    else
      hipLaunchKernelGGL(scan_decode_undistort_kernel<false>, dim3(tiles), dim3(256), 0, st, m, u, chain, S->d_points.as<float>(),
                         S->d_rgba.as<uint32_t>(), ctl + kScanTotal);
  }
  VGX_HIP(ctx, hipGetLastError());
  unsigned long long back[5] = {0, 0, 0, 0, 0};  // {error, total} and, undistorting, the three running counters
  VGX_HIP(ctx, hipMemcpyAsync(back, ctl + kScanError, tr ? 40 : 16, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  if (back[0] != 0) {
    (void)hipMemsetAsync(ctl + kScanError, 0, 8, st);
    return set_error(ctx, VGX_ERR_HIP, "scan: a tile of the decode never reported (internal error)");
  }
  S->n_points = (int64_t)back[1];
  S->n_dropped = (int64_t)n - S->n_points;
  if (tr) {
    S->n_bad_time = (int64_t)(back[2] - S->counters_base[0]);
    S->n_overflowed = (int64_t)(back[3] - S->counters_base[1]);
    S->n_clamped = (int64_t)(back[4] - S->counters_base[2]);
    for (int k = 0; k < 3; ++k) S->counters_base[k] = back[2 + k];
    S->counters_known = true;
  }
  return VGX_OK;
}

// f, tr: the undistorting decode's time field and track; both NULL for the plain decode
int scan_decode(const char* fn, vgx_scan S, const vgx_scan_layout* l, const vgx_scan_config* cfg, bool undistort,
                const vgx_scan_time_field* f, const vgx_scan_track* tr, const void* data, int64_t n_bytes, bool on_device) {
  if (!S) return VGX_ERR_INVALID;
  vgx_ctx ctx = S->ctx;
  vgx_scan_config c;
  vgx_scan_config_default(&c);
  if (cfg) c = *cfg;
  std::string why;
  int rc = undistort ? scan_undistort_check(l, &c, f, tr, n_bytes, &why) : scan_check(l, &c, n_bytes, &why);
  const size_t n = rc == VGX_OK ? (size_t)l->width * l->height : 0;
  if (rc == VGX_OK && n > 0 && !data) {
    rc = VGX_ERR_INVALID;
    why = "NULL data";
  }
  if (rc != VGX_OK) return set_error(ctx, rc, std::string(fn) + ": " + why);
  std::lock_guard<std::mutex> lk(S->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  S->n_points = S->n_dropped = 0;  // (what a failure below leaves: no scan)
  S->n_bad_time = S->n_overflowed = S->n_clamped = 0;
  S->depth_candidates = S->depth_invalid = S->depth_out_of_range = S->depth_overflowed = 0;
  if (n == 0) return VGX_OK;
  const uint8_t* d_data = static_cast<const uint8_t*>(data);
  if (!on_device) {
    const size_t bytes = (size_t)(l->height - 1) * l->row_step + (size_t)l->width * l->point_step;
    if (bytes > S->d_msg.bytes) {
      VGX_HIP(ctx, hipStreamSynchronize(ctx->tsdf_stream));
      const hipError_t e = S->d_msg.alloc(bytes);
      if (e != hipSuccess) return alloc_error(ctx, e, "scan: allocating the message");
    }
    rc = scan_upload(S, ctx->tsdf_stream, data, bytes);
    if (rc != VGX_OK) return rc;
    d_data = S->d_msg.as<uint8_t>();
  }
  return scan_decode_queued(S, *l, c, undistort ? f : nullptr, undistort ? tr : nullptr, d_data);
}

template <int ENC, bool ELEMENTS>
void depth_launch(hipStream_t st, uint32_t tiles, const DepthImage& m, const ScanDeskew* u, const TileChain& chain, float* points,
                  uint32_t* rgba, unsigned long long* total) {
  if (u)
    hipLaunchKernelGGL((depth_decode_undistort_kernel<ENC, ELEMENTS>), dim3(tiles), dim3(256), 0, st, m, *u, chain, points, rgba, total);
  else
    hipLaunchKernelGGL((depth_decode_kernel<ENC, ELEMENTS>), dim3(tiles), dim3(256), 0, st, m, chain, points, rgba, total);
}

// The decode of a depth image at d_depth with its colour image at d_color (device) on the TSDF stream; the caller holds
// S->mu and ctx->tsdf_mu, the device is set, everything has passed its check.  Ends with the call's one host
// synchronisation.
int depth_decode_queued(vgx_scan S, const vgx_depth_image_layout& l, const vgx_depth_camera& cam, const vgx_scan_config& c,
                        const vgx_depth_row_time* rt, const vgx_scan_track* tr, const uint8_t* d_depth, const uint8_t* d_color) {
  vgx_ctx ctx = S->ctx;
  hipStream_t st = ctx->tsdf_stream;
  const uint32_t su = (uint32_t)cam.stride_u, sv = (uint32_t)cam.stride_v;
  const uint32_t wc = (l.width - 1) / su + 1, hc = (l.height - 1) / sv + 1;  // (width, height >= 1 here)
  const uint32_t n = wc * hc;
  const uint32_t tiles = (n + kScanTile - 1) / kScanTile;
  int rc = scan_reserve(S, n, tiles);
  if (rc != VGX_OK) return rc;
  unsigned long long* ctl = S->d_ctl.as<unsigned long long>();
  DepthImage m{};
  m.depth = d_depth;
  m.color = d_color;
  m.n = n;
  m.wc = wc;
  m.wc_magic = wc >= 2u ? ~0ull / wc + 1ull : 0ull;
  m.row_step = l.row_step;
  m.color_row_step = l.color_kind == VGX_IMAGE_COLOR_NONE ? 0u : l.color_row_step;
  m.stride_u = su;
  m.stride_v = sv;
  m.color_kind = l.color_kind;
  m.unit = cam.depth_unit_m;
  m.min_z = cam.min_depth_m;
  m.max_z = cam.max_depth_m;
  m.cxf = (float)cam.cx;
  m.cyf = (float)cam.cy;
  m.kx = (float)(1.0 / cam.fx);
  m.ky = (float)(1.0 / cam.fy);
  std::memcpy(&m.constant, c.constant_rgba, 4);
  m.counters = ctl + kScanDepthInvalid;
  ScanDeskew u{};
  if (tr) {
    if ((rc = scan_track_upload(S, tr, &u)) != VGX_OK) return rc;
    u.scale = rt->scale;
    u.offset_s = rt->offset_s;
  }
  if ((rc = scan_counters_open(S)) != VGX_OK) return rc;
  const bool sixteen = l.encoding == VGX_DEPTH_16UC1;
  const bool elements = ((uintptr_t)d_depth | l.row_step) % (sixteen ? 2u : 4u) == 0;
  float* points = S->d_points.as<float>();
  uint32_t* rgba = S->d_rgba.as<uint32_t>();
  const ScanDeskew* up = tr ? &u : nullptr;
  // (the chain is taken right before the launch: nothing that can fail may come between)
  TileChain chain;
  if ((rc = scan_chain(S, tiles, &chain)) != VGX_OK) return rc;
  if (sixteen) {
    if (elements)
      depth_launch<VGX_DEPTH_16UC1, true>(st, tiles, m, up, chain, points, rgba, ctl + kScanTotal);
    else
      depth_launch<VGX_DEPTH_16UC1, false>(st, tiles, m, up, chain, points, rgba, ctl + kScanTotal);
  } else {
    if (elements)
      depth_launch<VGX_DEPTH_32FC1, true>(st, tiles, m, up, chain, points, rgba, ctl + kScanTotal);
    else
      depth_launch<VGX_DEPTH_32FC1, false>(st, tiles, m, up, chain, points, rgba, ctl + kScanTotal);
  }
  VGX_HIP(ctx, hipGetLastError());
  unsigned long long back[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // {error, total}, the track step's three running counters, the depth decode's three
  VGX_HIP(ctx, hipMemcpyAsync(back, ctl + kScanError, 64, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  if (back[0] != 0) {
    (void)hipMemsetAsync(ctl + kScanError, 0, 8, st);
    return set_error(ctx, VGX_ERR_HIP, "scan: a tile of the decode never reported (internal error)");
  }
  S->n_points = (int64_t)back[1];
  S->n_dropped = (int64_t)n - S->n_points;
  S->depth_candidates = (int64_t)n;
  if (tr) {
    S->n_bad_time = (int64_t)(back[2] - S->counters_base[0]);
    S->n_overflowed = (int64_t)(back[3] - S->counters_base[1]);
    S->n_clamped = (int64_t)(back[4] - S->counters_base[2]);
  }
  S->depth_invalid = (int64_t)(back[5] - S->depth_base[0]);
  S->depth_out_of_range = (int64_t)(back[6] - S->depth_base[1]);
  S->depth_overflowed = (int64_t)(back[7] - S->depth_base[2]);
  for (int k = 0; k < 3; ++k) {
    S->counters_base[k] = back[2 + k];
    S->depth_base[k] = back[5 + k];
  }
  S->counters_known = true;
  return VGX_OK;
}

// rt, tr: the undistorting decode's row time and track; both NULL for the plain decode
int depth_decode(const char* fn, vgx_scan S, const vgx_depth_image_layout* l, const vgx_depth_camera* cam, const vgx_scan_config* cfg,
                 bool undistort, const vgx_depth_row_time* rt, const vgx_scan_track* tr, const void* depth, int64_t depth_n_bytes,
                 const void* color, int64_t color_n_bytes, bool on_device) {
  if (!S) return VGX_ERR_INVALID;
  vgx_ctx ctx = S->ctx;
  vgx_scan_config c;
  vgx_scan_config_default(&c);
  if (cfg) c = *cfg;
  std::string why;
  int rc = undistort ? depth_undistort_check(l, cam, &c, rt, tr, depth_n_bytes, color_n_bytes, &why)
                     : depth_check(l, cam, &c, depth_n_bytes, color_n_bytes, &why);
  const size_t n = rc == VGX_OK ? (size_t)l->width * l->height : 0;
  if (rc == VGX_OK && n > 0 && !depth) {
    rc = VGX_ERR_INVALID;
    why = "NULL depth image";
  }
  if (rc == VGX_OK && n > 0 && l->color_kind != VGX_IMAGE_COLOR_NONE && !color) {
    rc = VGX_ERR_INVALID;
    why = "NULL colour image";
  }
  if (rc != VGX_OK) return set_error(ctx, rc, std::string(fn) + ": " + why);
  std::lock_guard<std::mutex> lk(S->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  S->n_points = S->n_dropped = 0;  // (what a failure below leaves: no scan)
  S->n_bad_time = S->n_overflowed = S->n_clamped = 0;
  S->depth_candidates = S->depth_invalid = S->depth_out_of_range = S->depth_overflowed = 0;
  if (n == 0) return VGX_OK;
  const bool colour = l->color_kind != VGX_IMAGE_COLOR_NONE;
  const uint8_t* d_depth = static_cast<const uint8_t*>(depth);
  const uint8_t* d_color = colour ? static_cast<const uint8_t*>(color) : nullptr;
  if (!on_device) {
    // both images into the handle's one upload buffer, the colour image at the next multiple of 16 bytes
    const size_t bytes = (size_t)(l->height - 1) * l->row_step + (size_t)l->width * depth_bpp(l->encoding);
    const size_t cbytes = colour ? (size_t)(l->height - 1) * l->color_row_step + (size_t)l->width * colour_bpp(l->color_kind) : 0;
    const size_t cat = (bytes + 15) & ~(size_t)15;
    if (cat + cbytes > S->d_msg.bytes) {
      VGX_HIP(ctx, hipStreamSynchronize(ctx->tsdf_stream));
      const hipError_t e = S->d_msg.alloc(cat + cbytes);
      if (e != hipSuccess) return alloc_error(ctx, e, "scan: allocating the images");
    }
    rc = scan_upload(S, ctx->tsdf_stream, depth, bytes);
    if (rc == VGX_OK && colour) rc = scan_upload(S, ctx->tsdf_stream, color, cbytes, cat);
    if (rc != VGX_OK) return rc;
    d_depth = S->d_msg.as<uint8_t>();
    d_color = colour ? d_depth + cat : nullptr;
  }
  return depth_decode_queued(S, *l, *cam, c, undistort ? rt : nullptr, undistort ? tr : nullptr, d_depth, d_color);
}

int scan_integrate(const char* fn, bool merged, vgx_tsdf_integrator I, const float T[7], vgx_scan S, int32_t freespace,
                   int64_t* n_updates) {
  vgx_ctx ctx = I ? I->ctx : (S ? S->ctx : nullptr);
  if (!I || !T || !S) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL argument");
  if (S->ctx != I->ctx) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": the scan belongs to another context");
  std::lock_guard<std::mutex> lk(S->mu);
  const int64_t n = S->n_points;
  const void* p = n > 0 ? S->d_points.p : nullptr;
  const void* col = n > 0 ? S->d_rgba.p : nullptr;
  return merged ? vgx_tsdf_integrate_merged_device(I, T, p, col, n, freespace, n_updates)
                : vgx_tsdf_integrate_device(I, T, p, col, n, freespace, n_updates);
}

}  // namespace

namespace vgx {
// vgx_depth_image_check with its reason, for the projective integrator (vgx_depth_image.h)
int depth_image_check(const vgx_depth_image_layout* l, const vgx_depth_camera* cam, int64_t depth_n_bytes, int64_t color_n_bytes,
                      std::string* why) {
  return depth_check(l, cam, nullptr, depth_n_bytes, color_n_bytes, why);
}
}  // namespace vgx

extern "C" {

void vgx_scan_config_default(vgx_scan_config* cfg) {
  if (!cfg) return;
  cfg->intensity_min = 0.0f;
  cfg->intensity_max = 10000.0f;  // color_map_->setMaxValue(10000.0) (pointcloud_integrator.cpp:14)
  std::memset(cfg->constant_rgba, 0, 4);
}

int vgx_scan_layout_check(const vgx_scan_layout* layout, int64_t n_bytes) { return scan_check(layout, nullptr, n_bytes, nullptr); }

int vgx_scan_undistort_check(const vgx_scan_layout* layout, const vgx_scan_time_field* time_field, const vgx_scan_track* track,
                             int64_t n_bytes) {
  return scan_undistort_check(layout, nullptr, time_field, track, n_bytes, nullptr);
}

int vgx_scan_create(vgx_ctx ctx, vgx_scan* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_scan_create: NULL argument");
  vgx_scan S = new vgx_scan_s;
  S->ctx = ctx;
  *out = S;
  return VGX_OK;
}

int vgx_scan_destroy(vgx_scan S) {
  if (!S) return VGX_ERR_INVALID;
  vgx_ctx ctx = S->ctx;
  {
    std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->tsdf_stream);  // (a queued scan may still read the arrays)
  }
  delete S;
  return VGX_OK;
}

int vgx_scan_decode_msg(vgx_scan S, const vgx_scan_layout* layout, const vgx_scan_config* cfg, const void* data, int64_t n_bytes) {
  return scan_decode("vgx_scan_decode_msg", S, layout, cfg, false, nullptr, nullptr, data, n_bytes, false);
}

int vgx_scan_decode_msg_device(vgx_scan S, const vgx_scan_layout* layout, const vgx_scan_config* cfg, const void* d_data,
                               int64_t n_bytes) {
  return scan_decode("vgx_scan_decode_msg_device", S, layout, cfg, false, nullptr, nullptr, d_data, n_bytes, true);
}

int vgx_scan_decode_msg_undistorted(vgx_scan S, const vgx_scan_layout* layout, const vgx_scan_config* cfg,
                                    const vgx_scan_time_field* time_field, const vgx_scan_track* track, const void* data,
                                    int64_t n_bytes) {
  return scan_decode("vgx_scan_decode_msg_undistorted", S, layout, cfg, true, time_field, track, data, n_bytes, false);
}

int vgx_scan_decode_msg_undistorted_device(vgx_scan S, const vgx_scan_layout* layout, const vgx_scan_config* cfg,
                                           const vgx_scan_time_field* time_field, const vgx_scan_track* track, const void* d_data,
                                           int64_t n_bytes) {
  return scan_decode("vgx_scan_decode_msg_undistorted_device", S, layout, cfg, true, time_field, track, d_data, n_bytes, true);
}

int vgx_scan_undistort_stats(vgx_scan S, int64_t* n_bad_time, int64_t* n_overflowed, int64_t* n_clamped) {
  if (!S) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(S->mu);
  if (n_bad_time) *n_bad_time = S->n_bad_time;
  if (n_overflowed) *n_overflowed = S->n_overflowed;
  if (n_clamped) *n_clamped = S->n_clamped;
  return VGX_OK;
}

void vgx_depth_camera_default(vgx_depth_camera* cam) {
  if (!cam) return;
  cam->fx = cam->fy = cam->cx = cam->cy = 0.0;  // (fx, fy have no default: a decode refuses zeros)
  cam->depth_unit_m = 0.001f;
  cam->min_depth_m = 0.0f;
  cam->max_depth_m = INFINITY;
  cam->stride_u = cam->stride_v = 1;
}

int vgx_depth_image_check(const vgx_depth_image_layout* layout, const vgx_depth_camera* camera, int64_t depth_n_bytes,
                          int64_t color_n_bytes) {
  return depth_check(layout, camera, nullptr, depth_n_bytes, color_n_bytes, nullptr);
}

int vgx_depth_image_undistort_check(const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                    const vgx_depth_row_time* row_time, const vgx_scan_track* track, int64_t depth_n_bytes,
                                    int64_t color_n_bytes) {
  return depth_undistort_check(layout, camera, nullptr, row_time, track, depth_n_bytes, color_n_bytes, nullptr);
}

int vgx_scan_decode_depth_image(vgx_scan S, const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                const vgx_scan_config* cfg, const void* depth, int64_t depth_n_bytes, const void* color,
                                int64_t color_n_bytes) {
  return depth_decode("vgx_scan_decode_depth_image", S, layout, camera, cfg, false, nullptr, nullptr, depth, depth_n_bytes, color,
                      color_n_bytes, false);
}

int vgx_scan_decode_depth_image_device(vgx_scan S, const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                       const vgx_scan_config* cfg, const void* d_depth, int64_t depth_n_bytes, const void* d_color,
                                       int64_t color_n_bytes) {
  return depth_decode("vgx_scan_decode_depth_image_device", S, layout, camera, cfg, false, nullptr, nullptr, d_depth, depth_n_bytes,
                      d_color, color_n_bytes, true);
}

int vgx_scan_decode_depth_image_undistorted(vgx_scan S, const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                            const vgx_scan_config* cfg, const vgx_depth_row_time* row_time,
                                            const vgx_scan_track* track, const void* depth, int64_t depth_n_bytes, const void* color,
                                            int64_t color_n_bytes) {
  return depth_decode("vgx_scan_decode_depth_image_undistorted", S, layout, camera, cfg, true, row_time, track, depth, depth_n_bytes,
                      color, color_n_bytes, false);
}

int vgx_scan_decode_depth_image_undistorted_device(vgx_scan S, const vgx_depth_image_layout* layout, const vgx_depth_camera* camera,
                                                   const vgx_scan_config* cfg, const vgx_depth_row_time* row_time,
                                                   const vgx_scan_track* track, const void* d_depth, int64_t depth_n_bytes,
                                                   const void* d_color, int64_t color_n_bytes) {
  return depth_decode("vgx_scan_decode_depth_image_undistorted_device", S, layout, camera, cfg, true, row_time, track, d_depth,
                      depth_n_bytes, d_color, color_n_bytes, true);
}

int vgx_scan_depth_stats(vgx_scan S, int64_t* n_candidates, int64_t* n_invalid, int64_t* n_out_of_range, int64_t* n_overflowed) {
  if (!S) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(S->mu);
  if (n_candidates) *n_candidates = S->depth_candidates;
  if (n_invalid) *n_invalid = S->depth_invalid;
  if (n_out_of_range) *n_out_of_range = S->depth_out_of_range;
  if (n_overflowed) *n_overflowed = S->depth_overflowed;
  return VGX_OK;
}

int vgx_scan_stats(vgx_scan S, int64_t* n_points, int64_t* n_dropped) {
  if (!S) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(S->mu);
  if (n_points) *n_points = S->n_points;
  if (n_dropped) *n_dropped = S->n_dropped;
  return VGX_OK;
}

int vgx_scan_device_pointers(vgx_scan S, const void** d_points, const void** d_rgba) {
  if (!S) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(S->mu);
  const bool any = S->n_points > 0;
  if (d_points) *d_points = any ? S->d_points.p : nullptr;
  if (d_rgba) *d_rgba = any ? S->d_rgba.p : nullptr;
  return VGX_OK;
}

int vgx_scan_download(vgx_scan S, float* points, uint8_t* rgba) {
  if (!S) return VGX_ERR_INVALID;
  vgx_ctx ctx = S->ctx;
  std::lock_guard<std::mutex> lk(S->mu);
  if (S->n_points == 0) return VGX_OK;
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->tsdf_stream;
  const size_t n = (size_t)S->n_points;
  if (points) VGX_HIP(ctx, hipMemcpyAsync(points, S->d_points.p, n * 12, hipMemcpyDeviceToHost, st));
  if (rgba) VGX_HIP(ctx, hipMemcpyAsync(rgba, S->d_rgba.p, n * 4, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  return VGX_OK;
}

int vgx_tsdf_integrate_scan(vgx_tsdf_integrator I, const float T[7], vgx_scan S, int32_t freespace, int64_t* n_updates) {
  return scan_integrate("vgx_tsdf_integrate_scan", false, I, T, S, freespace, n_updates);
}

int vgx_tsdf_integrate_merged_scan(vgx_tsdf_integrator I, const float T[7], vgx_scan S, int32_t freespace, int64_t* n_updates) {
  return scan_integrate("vgx_tsdf_integrate_merged_scan", true, I, T, S, freespace, n_updates);
}

}  // extern "C"
