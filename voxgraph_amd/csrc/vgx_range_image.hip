// LiDAR range images (include/voxgraph_amd.h, "LiDAR range images"): a scan's points gathered into a spherical
// image -- the nearest return per pixel, of equal ranges the lowest index, by ONE atomicMin per point on a 64-bit key -- and
// the projective integration of that image: the block walk of vgx_projective_kernel.h with a spherical frame.
//
// Build: a memset and two launches.  scatter: one lane per point, key = bits(r) << 32 | index into the pixel's cell (a
// positive float's bits order as the float does: the order the lanes run in cannot show).  resolve: one lane per cell, the
// winner's range and colour into the cell the integrator reads, its index beside it, and the reductions the candidate box
// needs (filled cells, largest range, extremes of the winning points and of their unit directions: integer sums and min /
// max, order-free).  Integration: one launch, no upload -- the image is resident.
//
// Two sensor models share all of it but the pixel rule: uniform rows (vgx_lidar_model) and a beam table
// (vgx_lidar_beam_model, DESIGN.md 32: rows with boundaries and an azimuth offset of their own, kept on the device by the
// image and uploaded only when the table changes).  The scatter kernel and the frame are templates over the device model.
#include <cmath>
#include <cstring>
#include <string>

#include "vgx_projective_kernel.h"

#pragma clang fp contract(off)

namespace vgx {

// the angle rule (the header's vgx_atan2_rule): an explicit f32 operation sequence, the same on the host and the device
__host__ __device__ __forceinline__ float atan2_rule(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  if (!(mx > 0.0f)) return 0.0f;
  const float q = mn / mx;
  const float s = q * q;
  float p = VGX_ATAN2_C5;
  p = p * s + VGX_ATAN2_C4;
  p = p * s + VGX_ATAN2_C3;
  p = p * s + VGX_ATAN2_C2;
  p = p * s + VGX_ATAN2_C1;
  p = p * s + VGX_ATAN2_C0;
  float a = p * q;
  if (ay > ax) a = VGX_ATAN2_PI_2 - a;
  if (x < 0.0f) a = VGX_ATAN2_PI - a;
  if (y < 0.0f) a = -a;
  return a;
}

struct RangeModelDev {
  int32_t width, height;
  float az_first, su, el_first, sv;
};

// the pixel of a direction whose range is positive and finite; false: outside the rows
__host__ __device__ __forceinline__ bool range_pixel(const RangeModelDev& m, float x, float y, float z, int& ui, int& vi) {
  const float rho = sqrtf(x * x + y * y);
  const float az = atan2_rule(y, x), el = atan2_rule(z, rho);
  float ua = (az - m.az_first) * m.su + 0.5f;
  const float w = (float)m.width;
  if (ua < 0.0f) ua += w;
  else if (ua >= w) ua -= w;
  ui = (int)floorf(ua);
  ui = ui < 0 ? 0 : (ui > m.width - 1 ? m.width - 1 : ui);
  const float va = (el - m.el_first) * m.sv + 0.5f;
  if (!(va >= 0.0f && va < (float)m.height)) return false;
  vi = (int)floorf(va);
  return true;
}

// ---- a beam table (the header's vgx_lidar_beam_model): rows with boundaries of their own and an azimuth
// offset each.  The rows are held in ASCENDING elevation, one 16-byte record a row, so that the boundary compares and the
// offset come with one load.
constexpr int kBeamMaxRows = 256;
constexpr int kBeamBins = 256;  // of the coarse table in front of the row walk
struct BeamModelDev {
  int32_t width, height;
  float az_first, su;
  float lo0;            // rows[0].x
  float bin_scale;      // bins per radian from lo0 on
  int32_t descending;   // the table's row 0 is the highest: vi = height - 1 - k
  const float4* rows;   // [height] {lo, hi, off, 0}, lo ascending
  const uint8_t* first; // [kBeamBins]: a row k with lo_k <= el for every el the bin can hold
};

// The row search: k = the largest row with lo_k <= el (the rule is stated without the search: any search gives that row).
// The bin of el gives a row at or below the answer, then the next three rows are compared at once: two dependent loads
// unless more than three rows start within two bins.  (Measured against a binary search over the rows)
__host__ __device__ __forceinline__ bool beam_row(const BeamModelDev& m, float el, int& k, float& off) {
  if (!(m.lo0 <= el)) return false;  // below the lowest row: there is no k
  const float t = (el - m.lo0) * m.bin_scale;  // >= 0; the host table allows for a whole bin of rounding
  int a = m.first[t < (float)(kBeamBins - 1) ? (int)t : kBeamBins - 1];
  float4 r = m.rows[a];
  const int last = m.height - 1;
  for (;;) {
    const float4 r1 = m.rows[a + 1 < last ? a + 1 : last], r2 = m.rows[a + 2 < last ? a + 2 : last], r3 = m.rows[a + 3 < last ? a + 3 : last];
    const bool p1 = a + 1 <= last && r1.x <= el, p2 = p1 && a + 2 <= last && r2.x <= el, p3 = p2 && a + 3 <= last && r3.x <= el;
    if (p3) {
      a += 3;
      r = r3;
      continue;
    }
    if (p2) {
      a += 2;
      r = r2;
    } else if (p1) {
      a += 1;
      r = r1;
    }
    break;
  }
  if (!(el < r.y)) return false;     // above the row: in a gap, or above the highest row
  k = a;
  off = r.z;
  return true;
}

// the pixel of a direction whose range is positive and finite; false: outside the rows (the column needs the row's offset)
__host__ __device__ __forceinline__ bool range_pixel(const BeamModelDev& m, float x, float y, float z, int& ui, int& vi) {
  const float rho = sqrtf(x * x + y * y);
  const float az = atan2_rule(y, x), el = atan2_rule(z, rho);
  int k;
  float off;
  if (!beam_row(m, el, k, off)) return false;
  vi = m.descending ? m.height - 1 - k : k;
  float ua = ((az - m.az_first) - off) * m.su + 0.5f;
  const float w = (float)m.width;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {  // (|ua| <= 1.25 w + 0.5: one pass does not suffice)
    if (ua < 0.0f) ua += w;
    else if (ua >= w) ua -= w;
  }
  ui = (int)floorf(ua);
  ui = ui < 0 ? 0 : (ui > m.width - 1 ? m.width - 1 : ui);
  return true;
}

// u32 words of vgx_range_image_s::d_ctl.  Every word from kRiMaxRange on grows under atomicMax from 0: a largest value as
// its order-preserving key, a smallest one as the key's complement.
enum { kRiRejRange = 0, kRiRejRows = 1, kRiFilled = 2, kRiMaxRange = 3, kRiPointMin = 4, kRiPointMax = 7, kRiDirMin = 10, kRiDirMax = 13,
       kRiCtlWords = 16 };
constexpr int kRiExtremes = kRiCtlWords - kRiMaxRange;  // 13
constexpr int kRiCellsPerLane = 4;             // of the resolve kernel

// u32 keys that order as the floats do (negative floats: all bits flipped; others: the sign bit set)
__host__ __device__ __forceinline__ uint32_t float_key(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float key_float(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}

// (Model: RangeModelDev or BeamModelDev -- the pixel rule is the one difference)
template <class Model>
__global__ __launch_bounds__(256) void range_scatter_kernel(Model m, const float* __restrict__ points, uint32_t n,
                                                            unsigned long long* __restrict__ keys, uint32_t* __restrict__ ctl) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  int rejected = 0;  // 1 by range, 2 by row
  if (i < n) {
    const float x = points[3 * (size_t)i + 0], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
    const float r = norm3(x, y, z);
    int ui, vi;
    if (!(r > 0.0f && r < INFINITY)) rejected = 1;
    else if (!range_pixel(m, x, y, z, ui, vi)) rejected = 2;
    else  // (vi < height and ui < width by range_pixel: the cell exists)
      atomicMin(keys + (size_t)vi * (size_t)m.width + (size_t)ui, ((unsigned long long)__float_as_uint(r) << 32) | (unsigned long long)i);
  }
  // counted once per workgroup
  const int by_range = __syncthreads_count(rejected == 1), by_row = __syncthreads_count(rejected == 2);
  if (threadIdx.x == 0) {
    if (by_range) atomicAdd(ctl + kRiRejRange, (uint32_t)by_range);
    if (by_row) atomicAdd(ctl + kRiRejRows, (uint32_t)by_row);
  }
}

__global__ __launch_bounds__(256) void range_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ points,
                                                            const uint32_t* __restrict__ rgba, uint32_t n_cells,
                                                            unsigned long long* __restrict__ cells, int32_t* __restrict__ index,
                                                            uint32_t* __restrict__ ctl) {
  __shared__ uint32_t sh[4][kRiExtremes + 1];
  uint32_t e[kRiExtremes];
#pragma unroll
  for (int k = 0; k < kRiExtremes; ++k) e[k] = 0u;
  uint32_t count = 0;
  // (kRiCellsPerLane cells a lane, a workgroup's lanes on neighbouring cells: the 14 words below are what every workgroup
  // meets on, and fewer workgroups queue there for less long)
  for (int j = 0; j < kRiCellsPerLane; ++j) {
    const uint32_t i = (blockIdx.x * (uint32_t)kRiCellsPerLane + (uint32_t)j) * 256u + threadIdx.x;
    if (i >= n_cells) break;
    const unsigned long long key = keys[i];
    const bool filled = key != ~0ull;
    const uint32_t idx = (uint32_t)key;
    const float r = filled ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
    const uint32_t col = filled ? (rgba ? rgba[idx] : 0xffffffffu) : 0u;
    cells[i] = (unsigned long long)__float_as_uint(r) | ((unsigned long long)col << 32);
    index[i] = filled ? (int32_t)idx : -1;
    if (!filled) continue;
    ++count;
    const float p[3] = {points[3 * (size_t)idx + 0], points[3 * (size_t)idx + 1], points[3 * (size_t)idx + 2]};
    const uint32_t kr = __float_as_uint(r);  // (positive: its bits are its key)
    e[0] = kr > e[0] ? kr : e[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t kp = float_key(p[a]), kd = float_key(p[a] / r);
      uint32_t* at[4] = {&e[kRiPointMin - kRiMaxRange + a], &e[kRiPointMax - kRiMaxRange + a], &e[kRiDirMin - kRiMaxRange + a],
                         &e[kRiDirMax - kRiMaxRange + a]};
      const uint32_t v[4] = {~kp, kp, ~kd, kd};
#pragma unroll
      for (int q = 0; q < 4; ++q) *at[q] = v[q] > *at[q] ? v[q] : *at[q];
    }
  }
  // a wave's count and extremes, then the workgroup's, then one atomic per word
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) count += (uint32_t)__shfl_xor((int)count, d);
#pragma unroll
  for (int k = 0; k < kRiExtremes; ++k) {
    uint32_t v = e[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
      v = o > v ? o : v;
    }
    if (lane == 0) sh[wave][k] = v;
  }
  if (lane == 0) sh[wave][kRiExtremes] = count;
  __syncthreads();
  if (threadIdx.x < kRiExtremes) {
    uint32_t v = sh[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < 4; ++w) v = sh[w][threadIdx.x] > v ? sh[w][threadIdx.x] : v;
    if (v) atomicMax(ctl + kRiMaxRange + threadIdx.x, v);
  } else if (threadIdx.x == kRiExtremes) {
    const uint32_t total = sh[0][kRiExtremes] + sh[1][kRiExtremes] + sh[2][kRiExtremes] + sh[3][kRiExtremes];
    if (total) atomicAdd(ctl + kRiFilled, total);
  }
}

// the spherical frame of the block walk; Model: RangeModelDev (uniform rows) or BeamModelDev (a beam table) -- the pixel
// rule is the one difference, the cones are those of the outermost rows' outer boundaries either way
template <class Model>
struct SphericalFrame : ProjFrameBase {
  const unsigned long long* cells;  // [height][width] {range f32 (lo), rgba (hi)}
  Model m;
  float reach;                         // no voxel beyond this range can be updated (early reject only)
  float top_s, top_c, bot_s, bot_c;    // sine and cosine of the widened upper and lower cones' elevations

  // can any voxel of block (bx, by, bz) be updated?  (conservative: true when in doubt)
  __device__ __forceinline__ bool block_in_view(float block_size, int bx, int by, int bz) const {
    float x, y, z;
    const float r = block_sphere(*this, block_size, bx, by, bz, x, y, z);
    const float d = norm3(x, y, z);
    if (!(d > r)) return true;          // the sensor is inside the sphere
    if (d - r > reach) return false;    // wholly beyond the longest return, truncation included
    // in the (rho, z) half plane the sphere is a disc of at most its radius (rho is 1-Lipschitz); every point of it lies
    // above the upper cone when the centre is more than r on the upper side of the cone's line, below the lower alike
    const float rho = sqrtf(x * x + y * y);
    if (top_c * z - top_s * rho > r) return false;
    if (bot_s * rho - bot_c * z > r) return false;
    return true;
  }

  // the rules of the header, in its order
  __device__ __forceinline__ bool term(const vgx_tsdf_config& c, float vs, int vx, int vy, int vz, float& sdf, float& uw,
                                       uint32_t& color, int& kind) const {
    const float gx = ((float)vx + 0.5f) * vs, gy = ((float)vy + 0.5f) * vs, gz = ((float)vz + 0.5f) * vs;
    float x, y, z;
    to_camera(*this, gx, gy, gz, x, y, z);
    const float r_v = norm3(x, y, z);
    if (!(r_v > 0.0f && r_v < INFINITY)) return false;
    int ui, vi;
    if (!range_pixel(m, x, y, z, ui, vi)) return false;
    const unsigned long long cell = cells[(size_t)vi * (size_t)m.width + (size_t)ui];
    const float r_s = __uint_as_float((uint32_t)cell);
    if (!(r_s > 0.0f)) return false;  // an empty cell
    const float trunc = c.default_truncation_distance;
    sdf = r_s - r_v;
    kind = 0;
    if (r_s < c.min_ray_length_m) return false;
    if (r_s > c.max_ray_length_m) {
      if (!(c.allow_clear && c.voxel_carving_enabled && r_v + trunc <= c.max_ray_length_m)) return false;
      sdf = c.max_ray_length_m - r_v;
      kind = 2;
    } else {
      if (sdf < -trunc) return false;
      if (sdf > trunc) {
        if (!c.voxel_carving_enabled) return false;
        kind = 1;
      }
    }
    uw = c.use_const_weight ? 1.0f : 1.0f / (r_s * r_s);
    if (c.use_weight_dropoff && sdf < -vs) {  // update_term's drop-off (vgx_tsdf_det.hip)
      uw = uw * (trunc + sdf) / (trunc - vs);
      uw = fmaxf(uw, 0.0f);
    }
    color = (uint32_t)(cell >> 32);
    return true;
  }
};
using RangeFrame = SphericalFrame<RangeModelDev>;
using BeamFrame = SphericalFrame<BeamModelDev>;

constexpr double kTwoPi = 6.283185307179586, kHalfPi = 1.5707963267948966;

int range_model_check(const vgx_lidar_model* m, std::string* why) {
  auto fail = [why](int code, const char* msg) {
    if (why) *why = msg;
    return code;
  };
  if (!m) return fail(VGX_ERR_INVALID, "NULL model");
  if (!std::isfinite(m->azimuth_first_rad) || !std::isfinite(m->elevation_first_rad) || !std::isfinite(m->elevation_last_rad))
    return fail(VGX_ERR_INVALID, "an angle is not finite");
  if (m->width < 1 || m->height < 1) return fail(VGX_ERR_INVALID, "width or height is less than 1");
  if (std::fabs(m->azimuth_first_rad) > VGX_ATAN2_PI) return fail(VGX_ERR_INVALID, "azimuth_first_rad lies outside [-pi, pi]");
  if (!(std::fabs((double)m->elevation_first_rad) < kHalfPi) || !(std::fabs((double)m->elevation_last_rad) < kHalfPi))
    return fail(VGX_ERR_INVALID, "an elevation lies outside (-pi/2, pi/2)");
  if (m->height > 1 && m->elevation_first_rad == m->elevation_last_rad)
    return fail(VGX_ERR_INVALID, "elevation_first_rad equals elevation_last_rad");
  if (m->width > 4096 || m->height > 256) return fail(VGX_ERR_UNSUPPORTED, "width is more than 4096 or height more than 256");
  if (m->width < 4) return fail(VGX_ERR_UNSUPPORTED, "width is less than 4");
  if (m->height == 1) return fail(VGX_ERR_UNSUPPORTED, "a single row has no pitch");
  return VGX_OK;
}

RangeModelDev range_model_dev(const vgx_lidar_model& m) {
  RangeModelDev d;
  d.width = m.width;
  d.height = m.height;
  d.az_first = m.azimuth_first_rad;
  d.su = (float)((m.azimuth_clockwise ? -1.0 : 1.0) * (double)m.width / kTwoPi);
  d.el_first = m.elevation_first_rad;
  d.sv = (float)((double)(m.height - 1) / ((double)m.elevation_last_rad - (double)m.elevation_first_rad));
  return d;
}

double range_pitch_az(const vgx_lidar_model& m) { return kTwoPi / (double)m.width; }
double range_pitch_el(const vgx_lidar_model& m) {
  return std::fabs((double)m.elevation_last_rad - (double)m.elevation_first_rad) / (double)(m.height - 1);
}

// A beam table's derived constants (the header's "derived constants"): the rows in ASCENDING elevation
struct BeamTable {
  int32_t height = 0;
  bool descending = false;
  std::vector<float4> rows;     // {lo, hi, off, 0}: each boundary formed in f64, rounded once, then clamped to [-PI_2, PI_2]
  std::vector<uint8_t> first;   // [kBeamBins], see BeamModelDev
  float bin_scale = 0.0f;
  double ext_max = 0.0;         // max_k (double)hi_k - (double)lo_k
};

// VGX_OK and the derived table in *out (may be NULL), or why the model is refused
int beam_model_check(const vgx_lidar_beam_model* m, BeamTable* out, std::string* why) {
  auto fail = [why](int code, const char* msg) {
    if (why) *why = msg;
    return code;
  };
  if (!m || !m->row_elevation_rad) return fail(VGX_ERR_INVALID, "NULL model or NULL row_elevation_rad");
  if (m->width < 1 || m->height < 1) return fail(VGX_ERR_INVALID, "width or height is less than 1");
  if (!std::isfinite(m->azimuth_first_rad)) return fail(VGX_ERR_INVALID, "an angle is not finite");
  if (std::fabs(m->azimuth_first_rad) > VGX_ATAN2_PI) return fail(VGX_ERR_INVALID, "azimuth_first_rad lies outside [-pi, pi]");
  if (!(m->row_half_extent_max_rad > 0.0f)) return fail(VGX_ERR_INVALID, "row_half_extent_max_rad is not positive");
  if (m->height > kBeamMaxRows) {  // (read no further than the rows the rule can hold)
    return fail(VGX_ERR_UNSUPPORTED, "width is more than 4096 or height more than 256");
  }
  const int H = m->height;
  const float* e = m->row_elevation_rad;
  const bool descending = H > 1 && e[1] < e[0];
  for (int k = 0; k < H; ++k) {
    if (!std::isfinite(e[k]) || (m->row_azimuth_offset_rad && !std::isfinite(m->row_azimuth_offset_rad[k])))
      return fail(VGX_ERR_INVALID, "an angle is not finite");
    if (!(std::fabs((double)e[k]) < kHalfPi)) return fail(VGX_ERR_INVALID, "an elevation lies outside (-pi/2, pi/2)");
    if (m->row_azimuth_offset_rad && std::fabs(m->row_azimuth_offset_rad[k]) > VGX_ATAN2_PI_2)
      return fail(VGX_ERR_INVALID, "an azimuth offset lies outside [-pi/2, pi/2]");
    if (k > 0 && !(descending ? e[k] < e[k - 1] : e[k] > e[k - 1]))
      return fail(VGX_ERR_INVALID, "row_elevation_rad is not strictly monotone");
  }
  if (m->width > 4096) return fail(VGX_ERR_UNSUPPORTED, "width is more than 4096 or height more than 256");
  if (m->width < 4) return fail(VGX_ERR_UNSUPPORTED, "width is less than 4");
  const double L = (double)m->row_half_extent_max_rad;
  if (H == 1 && std::isinf(L)) return fail(VGX_ERR_INVALID, "a single row needs a finite row_half_extent_max_rad");
  BeamTable t;
  t.height = H;
  t.descending = descending;
  t.rows.resize((size_t)H);
  auto s = [&](int k) { return (double)e[descending ? H - 1 - k : k]; };
  auto once = [](double v) { return std::fmin(std::fmax((float)v, -VGX_ATAN2_PI_2), VGX_ATAN2_PI_2); };
  for (int k = 0; k < H; ++k) {
    double lo, hi;
    if (H == 1) {
      lo = s(0) - L;
      hi = s(0) + L;
    } else {
      const double below = k > 0 ? (s(k - 1) + s(k)) * 0.5 : 0.0, above = k < H - 1 ? (s(k) + s(k + 1)) * 0.5 : 0.0;
      lo = k > 0 ? std::fmax(below, s(k) - L) : s(0) - std::fmin(above - s(0), L);
      hi = k < H - 1 ? std::fmin(above, s(k) + L) : s(k) + std::fmin(s(k) - below, L);
    }
    const int row = descending ? H - 1 - k : k;
    t.rows[(size_t)k] = make_float4(once(lo), once(hi), m->row_azimuth_offset_rad ? m->row_azimuth_offset_rad[row] : 0.0f, 0.0f);
  }
  for (int k = 0; k < H; ++k) {
    if (!(t.rows[k].x < t.rows[k].y) || (k + 1 < H && !(t.rows[k].y <= t.rows[k + 1].x)))
      return fail(VGX_ERR_INVALID, "the rounded row boundaries do not leave every row an extent");
    t.ext_max = std::fmax(t.ext_max, (double)t.rows[k].y - (double)t.rows[k].x);
  }
  // the coarse table: kBeamBins bins from lo_0 to hi_{H-1}; a bin's entry is the largest row whose lo is at or below the
  // lower edge of the bin BEFORE it -- the f32 bin index of an elevation is off by far less than one bin (two roundings of
  // 2^-24 on a value below 256), so the entry's lo never exceeds the elevation
  const double lo0 = (double)t.rows[0].x, span = (double)t.rows[(size_t)H - 1].y - lo0;
  t.bin_scale = std::fmin((float)((double)kBeamBins / span), 1e6f);
  t.first.assign((size_t)kBeamBins, 0);
  for (int b = 1, k = 0; b < kBeamBins; ++b) {
    const double edge = lo0 + (double)(b - 1) / (double)t.bin_scale;
    while (k + 1 < H && (double)t.rows[(size_t)k + 1].x <= edge) ++k;
    t.first[(size_t)b] = (uint8_t)k;
  }
  if (out) *out = std::move(t);
  return VGX_OK;
}

// the by-value part of the device model; rows and first point where the caller says (host or device memory)
BeamModelDev beam_model_dev(const vgx_lidar_beam_model& m, const BeamTable& t, const float4* rows, const uint8_t* first) {
  BeamModelDev d;
  d.width = m.width;
  d.height = m.height;
  d.az_first = m.azimuth_first_rad;
  d.su = (float)((m.azimuth_clockwise ? -1.0 : 1.0) * (double)m.width / kTwoPi);
  d.lo0 = t.rows[0].x;
  d.bin_scale = t.bin_scale;
  d.descending = t.descending ? 1 : 0;
  d.rows = rows;
  d.first = first;
  return d;
}

// The candidate block box, f64 throughout (the header's "candidates").
// pitch_el: the uniform rows' pitch, or a beam table's largest row extent
int range_image_box(double pitch_az, double pitch_el, const vgx_range_image_counts& ic, const vgx_tsdf_config& c, const float T[7],
                    float voxel_size, int32_t vps, int32_t lo[3], int32_t hi[3], std::string* why) {
  auto fail = [why](int code, const char* msg) {
    if (why) *why = msg;
    return code;
  };
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(T[k])) return fail(VGX_ERR_INVALID, "T_G_S is not finite");
  if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size) || (vps != 8 && vps != 16))
    return fail(VGX_ERR_INVALID, "voxel_size is not positive or voxels_per_side is not 8 or 16");
  const double trunc = (double)c.default_truncation_distance, max_ray = (double)c.max_ray_length_m;
  const double reach = std::fmin(max_ray, (double)ic.max_range) + trunc;
  if (!std::isfinite(reach) || !(reach >= 0.0)) return fail(VGX_ERR_UNSUPPORTED, "the reach is not finite");
  double blo[3] = {0.0, 0.0, 0.0}, bhi[3] = {0.0, 0.0, 0.0};
  if (ic.n_filled > 0) {
    for (int a = 0; a < 3; ++a) {
      const double pmax = (double)ic.point_max[a], pmin = (double)ic.point_min[a], dmax = (double)ic.dir_max[a], dmin = (double)ic.dir_min[a];
      // (an unbounded max_ray_length_m pulls nothing in: the point's extreme alone)
      const double in_hi = std::isfinite(max_ray) ? std::fmin(pmax, dmax * max_ray) : pmax;
      const double in_lo = std::isfinite(max_ray) ? std::fmax(pmin, dmin * max_ray) : pmin;
      bhi[a] = std::fmax(0.0, in_hi) + trunc * std::fmax(0.0, dmax);
      blo[a] = std::fmin(0.0, in_lo) + trunc * std::fmin(0.0, dmin);
    }
  }
  const double widen = reach * (pitch_az + pitch_el + 4.0 * (double)VGX_ATAN2_RULE_MAX_ERROR);
  const double bs = (double)voxel_size * (double)vps;
  const double qw = T[0], qx = T[1], qy = T[2], qz = T[3];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int corner = 0; corner < 8; ++corner) {
    const double px = (corner & 1) ? bhi[0] : blo[0], py = (corner & 2) ? bhi[1] : blo[1], pz = (corner & 4) ? bhi[2] : blo[2];
    double uvx = qy * pz - qz * py, uvy = qz * px - qx * pz, uvz = qx * py - qy * px;
    uvx += uvx; uvy += uvy; uvz += uvz;
    const double ccx = qy * uvz - qz * uvy, ccy = qz * uvx - qx * uvz, ccz = qx * uvy - qy * uvx;
    const double g[3] = {(px + qw * uvx + ccx) + (double)T[4], (py + qw * uvy + ccy) + (double)T[5], (pz + qw * uvz + ccz) + (double)T[6]};
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::fmin(mn[a], g[a]);
      mx[a] = std::fmax(mx[a], g[a]);
    }
  }
  for (int a = 0; a < 3; ++a) {
    const double flo = std::floor((mn[a] - widen) / bs) - 1.0, fhi = std::floor((mx[a] + widen) / bs) + 1.0;
    if (!(flo > -1073741824.0 && fhi < 1073741824.0)) return fail(VGX_ERR_UNSUPPORTED, "the candidate box exceeds +-2^30 blocks");
    lo[a] = (int32_t)flo;
    hi[a] = (int32_t)fhi;
  }
  return VGX_OK;
}

}  // namespace vgx

using namespace vgx;

struct vgx_range_image_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;  // taken before a scan's, an integrator's and ctx->tsdf_mu
  bool built = false;
  vgx_lidar_model model{};  // of a table image: the shared fields, the table's first and last elevation
  RangeModelDev dev{};
  // a table image (vgx_range_image_build_beams): the table as it was given, and what the kernels read
  bool is_table = false;
  std::vector<float> row_elevation, row_offset;  // [height]
  float row_limit = 0.0f;
  BeamModelDev beam_dev{};
  double beam_ext_max = 0.0;
  float beam_lo_first = 0.0f, beam_hi_last = 0.0f;
  bool table_resident = false;  // d_table holds the table of row_elevation, row_offset and row_limit
  DeviceBuffer d_table;         // kBeamMaxRows rows of 16 bytes, then kBeamBins bytes: allocated once, never moved
  UploadStage table_stage;      // the upload's pinned staging: outlives the copy
  DeviceBuffer d_keys;   // u64 [cells]: the scatter's keys
  DeviceBuffer d_cells;  // u64 [cells]: {range, rgba}, what the integrator reads
  DeviceBuffer d_index;  // i32 [cells]: the winning point, -1 empty
  DeviceBuffer d_ctl;    // u32 [kRiCtlWords]
  bool pending = false;  // the counts of the build queued last have not been read yet
  vgx_range_image_counts counts{};
};

namespace {

// the read-back of a queued build (the caller holds the image's lock and ctx->tsdf_mu)
int range_image_finish(vgx_range_image R) {
  if (!R->pending) return VGX_OK;
  vgx_ctx ctx = R->ctx;
  uint32_t back[kRiCtlWords] = {};
  VGX_HIP(ctx, hipMemcpyAsync(back, R->d_ctl.p, sizeof(back), hipMemcpyDeviceToHost, ctx->tsdf_stream));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->tsdf_stream));
  vgx_range_image_counts& c = R->counts;
  c.n_rejected_range = back[kRiRejRange];
  c.n_rejected_rows = back[kRiRejRows];
  c.n_kept = c.n_points - c.n_rejected_range - c.n_rejected_rows;
  c.n_filled = back[kRiFilled];
  c.n_collided = c.n_kept - c.n_filled;
  const bool any = c.n_filled > 0;
  std::memcpy(&c.max_range, &back[kRiMaxRange], 4);
  for (int a = 0; a < 3; ++a) {
    c.point_min[a] = any ? key_float(~back[kRiPointMin + a]) : INFINITY;
    c.point_max[a] = any ? key_float(back[kRiPointMax + a]) : -INFINITY;
    c.dir_min[a] = any ? key_float(~back[kRiDirMin + a]) : INFINITY;
    c.dir_max[a] = any ? key_float(back[kRiDirMax + a]) : -INFINITY;
  }
  R->pending = false;
  return VGX_OK;
}

constexpr size_t kBeamTableBytes = (size_t)kBeamMaxRows * sizeof(float4) + (size_t)kBeamBins;

// a beam table onto the device, unless the image holds it already (the caller holds the image's lock and ctx->tsdf_mu).  On
// the TSDF stream: a queued frame that still reads the table held is ordered before the copy.
int range_image_table(vgx_range_image R, const vgx_lidar_beam_model& m, const BeamTable& t) {
  vgx_ctx ctx = R->ctx;
  hipStream_t st = ctx->tsdf_stream;
  const size_t H = (size_t)m.height;
  std::vector<float> off(H, 0.0f);
  if (m.row_azimuth_offset_rad) off.assign(m.row_azimuth_offset_rad, m.row_azimuth_offset_rad + H);
  const bool same = R->table_resident && R->row_limit == m.row_half_extent_max_rad && R->row_elevation.size() == H &&
                    std::memcmp(R->row_elevation.data(), m.row_elevation_rad, H * 4) == 0 &&
                    std::memcmp(R->row_offset.data(), off.data(), H * 4) == 0;
  if (same) return VGX_OK;
  R->table_resident = false;
  if (!R->d_table.p) {
    hipError_t e = R->d_table.alloc(kBeamTableBytes);
    if (e == hipSuccess) e = R->table_stage.reserve(kBeamTableBytes);
    if (e != hipSuccess) {
      R->d_table.release();
      return alloc_error(ctx, e, "range image: allocating the beam table");
    }
  }
  int half = 0;
  hipError_t waited = hipSuccess;
  unsigned char* stage = static_cast<unsigned char*>(R->table_stage.next(&half, &waited));
  VGX_HIP(ctx, waited);
  std::memcpy(stage, t.rows.data(), H * sizeof(float4));
  std::memcpy(stage + (size_t)kBeamMaxRows * sizeof(float4), t.first.data(), (size_t)kBeamBins);
  VGX_HIP(ctx, hipMemcpyAsync(R->d_table.p, stage, kBeamTableBytes, hipMemcpyHostToDevice, st));
  VGX_HIP(ctx, R->table_stage.record(half, st));
  R->row_elevation.assign(m.row_elevation_rad, m.row_elevation_rad + H);
  R->row_offset = off;
  R->row_limit = m.row_half_extent_max_rad;
  R->table_resident = true;
  return VGX_OK;
}

// the caller holds the image's lock (and the scan's, where the arrays are a scan's); exactly one of model and beams is given
int range_image_build(const char* fn, vgx_range_image R, const vgx_lidar_model* model, const vgx_lidar_beam_model* beams,
                      const float* d_points, const uint32_t* d_rgba, int64_t n, vgx_range_image_counts* counts) {
  vgx_ctx ctx = R->ctx;
  std::string why;
  BeamTable table;
  const int rc = beams ? beam_model_check(beams, &table, &why) : range_model_check(model, &why);
  if (rc != VGX_OK) return set_error(ctx, rc, std::string(fn) + ": " + why);
  const int32_t width = beams ? beams->width : model->width, height = beams ? beams->height : model->height;
  if (n < 0 || (n > 0 && !d_points)) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL points or a negative count");
  if (n > (int64_t)INT32_MAX) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": more than 2^31 - 1 points");
  std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->tsdf_stream;
  const size_t n_cells = (size_t)width * (size_t)height;
  if (n_cells * 8 > R->d_keys.bytes || !R->d_ctl.p) {
    VGX_HIP(ctx, hipStreamSynchronize(st));  // (a queued frame may still read the cells)
    R->built = false;
    const hipError_t e = alloc_group({{&R->d_keys, n_cells * 8}, {&R->d_cells, n_cells * 8}, {&R->d_index, n_cells * 4},
                                      {&R->d_ctl, (size_t)kRiCtlWords * 4}});
    if (e != hipSuccess) return alloc_error(ctx, e, "range image: allocating the cells");
  }
  if (beams) {
    const int rt = range_image_table(R, *beams, table);
    if (rt != VGX_OK) {
      R->built = false;
      return rt;
    }
    R->model = vgx_lidar_model{width, height, beams->azimuth_first_rad, beams->azimuth_clockwise, beams->row_elevation_rad[0],
                               beams->row_elevation_rad[height - 1]};
    R->beam_dev = beam_model_dev(*beams, table, R->d_table.as<float4>(),
                                 R->d_table.as<uint8_t>() + (size_t)kBeamMaxRows * sizeof(float4));
    R->beam_ext_max = table.ext_max;
    R->beam_lo_first = table.rows.front().x;
    R->beam_hi_last = table.rows.back().y;
  } else {
    R->model = *model;
    R->dev = range_model_dev(*model);
  }
  R->is_table = beams != nullptr;
  R->counts = vgx_range_image_counts{};
  R->counts.n_points = n;
  VGX_HIP(ctx, hipMemsetAsync(R->d_keys.p, 0xff, n_cells * 8, st));
  VGX_HIP(ctx, hipMemsetAsync(R->d_ctl.p, 0, (size_t)kRiCtlWords * 4, st));
  uint32_t* ctl = R->d_ctl.as<uint32_t>();
  if (n > 0 && beams)
    hipLaunchKernelGGL(range_scatter_kernel<BeamModelDev>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, R->beam_dev, d_points,
                       (uint32_t)n, R->d_keys.as<unsigned long long>(), ctl);
  else if (n > 0)
    hipLaunchKernelGGL(range_scatter_kernel<RangeModelDev>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, R->dev, d_points,
                       (uint32_t)n, R->d_keys.as<unsigned long long>(), ctl);
  hipLaunchKernelGGL(range_resolve_kernel, dim3((unsigned)((n_cells + 256 * kRiCellsPerLane - 1) / (256 * kRiCellsPerLane))), dim3(256), 0, st,
                     R->d_keys.as<unsigned long long>(), d_points, d_rgba, (uint32_t)n_cells, R->d_cells.as<unsigned long long>(),
                     R->d_index.as<int32_t>(), ctl);
  VGX_HIP(ctx, hipGetLastError());
  R->built = true;
  R->pending = true;
  if (counts) {
    const int rf = range_image_finish(R);
    if (rf != VGX_OK) return rf;
    *counts = R->counts;
  }
  return VGX_OK;
}

// the frame of either kind of image, launched (the caller holds the image's, the integrator's and the TSDF lock).  e_top,
// e_bot: the elevations of the cones beyond which no voxel finds a row.
template <class Model>
int integrate_spherical(const char* fn, vgx_tsdf_integrator I, const float T[7], vgx_range_image R, const Model& dev, const int32_t lo[3],
                        const int32_t hi[3], double e_top, double e_bot, vgx_projective_counts* counts) {
  vgx_ctx ctx = I->ctx;
  vgx_tsdf_layer L = I->layer;
  const vgx_tsdf_config& c = I->dev.cfg;
  SphericalFrame<Model> f{};
  int rc = projective_begin(fn, I, lo, hi, &f);
  if (rc != VGX_OK) return rc;
  f.qw = T[0]; f.qx = T[1]; f.qy = T[2]; f.qz = T[3];
  f.tx = T[4]; f.ty = T[5]; f.tz = T[6];
  f.cells = R->d_cells.as<unsigned long long>();
  f.m = dev;
  f.reach = std::fmin(c.max_ray_length_m, R->counts.max_range) + c.default_truncation_distance;
  const bool top = e_top < kHalfPi - 1e-3, bot = e_bot > -kHalfPi + 1e-3;  // (a cone that closes on the axis rejects nothing)
  f.top_s = top ? (float)std::sin(e_top) : 1.0f;
  f.top_c = top ? (float)std::cos(e_top) : 0.0f;
  f.bot_s = bot ? (float)std::sin(e_bot) : -1.0f;
  f.bot_c = bot ? (float)std::cos(e_bot) : 0.0f;
  TileChain chain;
  rc = projective_chain(I, f, &chain);
  if (rc != VGX_OK) return rc;
  projective_launch(ctx->tsdf_stream, L->dev, c, f, chain, I->d_proj_ctl.as<unsigned long long>());
  return projective_end(fn, I, f, counts);
}

}  // namespace

extern "C" {

float vgx_atan2_rule(float y, float x) { return atan2_rule(y, x); }

int vgx_range_image_check(const vgx_lidar_model* model) { return range_model_check(model, nullptr); }

int vgx_range_image_pixel(const vgx_lidar_model* model, float x, float y, float z, int32_t* u, int32_t* v) {
  if (!u || !v || range_model_check(model, nullptr) != VGX_OK) return VGX_ERR_INVALID;
  const float r = sqrtf(x * x + y * y + z * z);
  if (!(r > 0.0f && r < INFINITY)) return VGX_ERR_INVALID;
  int ui = 0, vi = -1;
  if (!range_pixel(range_model_dev(*model), x, y, z, ui, vi)) vi = -1;  // (the column is defined whatever the row)
  *u = ui;
  *v = vi;
  return VGX_OK;
}

int vgx_range_image_create(vgx_ctx ctx, vgx_range_image* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_range_image_create: NULL argument");
  vgx_range_image R = new vgx_range_image_s;
  R->ctx = ctx;
  *out = R;
  return VGX_OK;
}

int vgx_range_image_destroy(vgx_range_image R) {
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  {
    std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->tsdf_stream);  // (a queued frame may still read the cells)
  }
  delete R;
  return VGX_OK;
}

namespace {
// the two builds from a scan handle
int build_from_scan(const char* fn, vgx_range_image R, const vgx_lidar_model* model, const vgx_lidar_beam_model* beams, vgx_scan scan,
                    vgx_range_image_counts* counts) {
  vgx_ctx ctx = R ? R->ctx : scan_context(scan);
  if (!R || !scan) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL argument");
  if (scan_context(scan) != ctx) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": the scan belongs to another context");
  std::lock_guard<std::mutex> own(R->mu);
  const float* d_points = nullptr;
  const uint32_t* d_rgba = nullptr;
  int64_t n = 0;
  // (the scan's lock until the launches are queued: a decode into the handle is then ordered behind them on the one stream)
  std::unique_lock<std::mutex> borrowed = scan_borrow(scan, &d_points, &d_rgba, &n);
  return range_image_build(fn, R, model, beams, d_points, d_rgba, n, counts);
}
}  // namespace

int vgx_range_image_build(vgx_range_image R, const vgx_lidar_model* model, vgx_scan scan, vgx_range_image_counts* counts) {
  return build_from_scan("vgx_range_image_build", R, model, nullptr, scan, counts);
}

int vgx_range_image_build_beams(vgx_range_image R, const vgx_lidar_beam_model* model, vgx_scan scan, vgx_range_image_counts* counts) {
  return build_from_scan("vgx_range_image_build_beams", R, nullptr, model, scan, counts);
}

int vgx_range_image_build_device(vgx_range_image R, const vgx_lidar_model* model, const void* d_points, const void* d_rgba, int64_t n,
                                 vgx_range_image_counts* counts) {
  if (!R) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> own(R->mu);
  return range_image_build("vgx_range_image_build_device", R, model, nullptr, static_cast<const float*>(d_points),
                           static_cast<const uint32_t*>(d_rgba), n, counts);
}

int vgx_range_image_build_beams_device(vgx_range_image R, const vgx_lidar_beam_model* model, const void* d_points, const void* d_rgba,
                                       int64_t n, vgx_range_image_counts* counts) {
  if (!R) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> own(R->mu);
  return range_image_build("vgx_range_image_build_beams_device", R, nullptr, model, static_cast<const float*>(d_points),
                           static_cast<const uint32_t*>(d_rgba), n, counts);
}

int vgx_range_image_beams(vgx_range_image R, int32_t* is_table, float* row_elevation, float* row_azimuth_offset,
                          float* row_half_extent_max_rad) {
  if (!R) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> own(R->mu);
  if (!R->built) return set_error(R->ctx, VGX_ERR_INVALID, "vgx_range_image_beams: no image built");
  if (is_table) *is_table = R->is_table ? 1 : 0;
  if (!R->is_table) return VGX_OK;
  if (row_elevation) std::memcpy(row_elevation, R->row_elevation.data(), R->row_elevation.size() * 4);
  if (row_azimuth_offset) std::memcpy(row_azimuth_offset, R->row_offset.data(), R->row_offset.size() * 4);
  if (row_half_extent_max_rad) *row_half_extent_max_rad = R->row_limit;
  return VGX_OK;
}

int vgx_range_image_stats(vgx_range_image R, vgx_range_image_counts* counts, vgx_lidar_model* model) {
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  std::lock_guard<std::mutex> own(R->mu);
  if (!R->built) return set_error(ctx, VGX_ERR_INVALID, "vgx_range_image_stats: no image built");
  {
    std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = range_image_finish(R);
    if (rc != VGX_OK) return rc;
  }
  if (counts) *counts = R->counts;
  if (model) *model = R->model;
  return VGX_OK;
}

int vgx_range_image_download(vgx_range_image R, float* range, uint8_t* rgba, int32_t* point_index) {
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  std::lock_guard<std::mutex> own(R->mu);
  if (!R->built) return set_error(ctx, VGX_ERR_INVALID, "vgx_range_image_download: no image built");
  std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->tsdf_stream;
  const size_t n_cells = (size_t)R->model.width * (size_t)R->model.height;
  std::vector<unsigned long long> cells(range || rgba ? n_cells : 0);  // (range and colour interleaved: taken apart here)
  if (!cells.empty()) VGX_HIP(ctx, hipMemcpyAsync(cells.data(), R->d_cells.p, n_cells * 8, hipMemcpyDeviceToHost, st));
  if (point_index) VGX_HIP(ctx, hipMemcpyAsync(point_index, R->d_index.p, n_cells * 4, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  for (size_t i = 0; i < cells.size(); ++i) {
    const uint32_t r = (uint32_t)cells[i], col = (uint32_t)(cells[i] >> 32);
    if (range) std::memcpy(range + i, &r, 4);
    if (rgba) std::memcpy(rgba + 4 * i, &col, 4);
  }
  return range_image_finish(R);
}

int vgx_tsdf_integrate_range_image(vgx_tsdf_integrator I, const float T[7], vgx_range_image R, vgx_projective_counts* counts) {
  const char* fn = "vgx_tsdf_integrate_range_image";
  vgx_ctx ctx = I ? I->ctx : (R ? R->ctx : nullptr);
  if (!I || !T || !R) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL argument");
  if (R->ctx != ctx) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": the image belongs to another context");
  std::lock_guard<std::mutex> image_lk(R->mu);
  std::lock_guard<std::mutex> own(I->mu);
  std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
  if (!I->layer) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": no layer set");
  if (!R->built) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": no image built");
  vgx_tsdf_layer L = I->layer;
  const vgx_tsdf_config& c = I->dev.cfg;
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = range_image_finish(R);  // (a queued build's counts: the box needs them)
  if (rc != VGX_OK) return rc;
  std::string why;
  int32_t lo[3], hi[3];
  const double pitch_el = R->is_table ? R->beam_ext_max : range_pitch_el(R->model);
  rc = range_image_box(range_pitch_az(R->model), pitch_el, R->counts, c, T, L->dev.voxel_size, L->dev.vps, lo, hi, &why);
  if (rc != VGX_OK) return set_error(ctx, rc, std::string(fn) + ": " + why);
  if (R->is_table) {
    // the cones of lo_0 and hi_{H-1}, widened by the rule's error and the rounding margin of the uniform frame
    const double margin = (double)VGX_ATAN2_RULE_MAX_ERROR + 1e-4 * R->beam_ext_max + 1e-5;
    return integrate_spherical(fn, I, T, R, R->beam_dev, lo, hi, (double)R->beam_hi_last + margin, (double)R->beam_lo_first - margin, counts);
  }
  // the rows' cones, widened by half a pitch, the rule's error and the f32 rounding of a row coordinate
  const double pitch = range_pitch_el(R->model);
  const double margin = 0.5 * pitch + (double)VGX_ATAN2_RULE_MAX_ERROR + 1e-4 * pitch + 1e-5;
  const double e_top = std::fmax((double)R->model.elevation_first_rad, (double)R->model.elevation_last_rad) + margin;
  const double e_bot = std::fmin((double)R->model.elevation_first_rad, (double)R->model.elevation_last_rad) - margin;
  return integrate_spherical(fn, I, T, R, R->dev, lo, hi, e_top, e_bot, counts);
}

int vgx_tsdf_range_image_box(const vgx_lidar_model* model, const vgx_range_image_counts* image_counts, const vgx_tsdf_config* cfg,
                             const float T_G_S[7], float voxel_size, int32_t voxels_per_side, int32_t lo[3], int32_t hi[3]) {
  if (!image_counts || !cfg || !T_G_S || !lo || !hi) return VGX_ERR_INVALID;
  const int rc = range_model_check(model, nullptr);
  if (rc != VGX_OK) return rc;
  return range_image_box(range_pitch_az(*model), range_pitch_el(*model), *image_counts, *cfg, T_G_S, voxel_size, voxels_per_side, lo, hi,
                         nullptr);
}

int vgx_range_image_check_beams(const vgx_lidar_beam_model* model) { return beam_model_check(model, nullptr, nullptr); }

int vgx_range_image_pixel_beams(const vgx_lidar_beam_model* model, float x, float y, float z, int32_t* u, int32_t* v) {
  BeamTable t;
  if (!u || !v || beam_model_check(model, &t, nullptr) != VGX_OK) return VGX_ERR_INVALID;
  const float r = sqrtf(x * x + y * y + z * z);
  if (!(r > 0.0f && r < INFINITY)) return VGX_ERR_INVALID;
  int ui = -1, vi = -1;
  if (!range_pixel(beam_model_dev(*model, t, t.rows.data(), t.first.data()), x, y, z, ui, vi)) ui = vi = -1;
  *u = ui;
  *v = vi;
  return VGX_OK;
}

int vgx_tsdf_range_image_box_beams(const vgx_lidar_beam_model* model, const vgx_range_image_counts* image_counts,
                                   const vgx_tsdf_config* cfg, const float T_G_S[7], float voxel_size, int32_t voxels_per_side,
                                   int32_t lo[3], int32_t hi[3]) {
  if (!image_counts || !cfg || !T_G_S || !lo || !hi) return VGX_ERR_INVALID;
  BeamTable t;
  const int rc = beam_model_check(model, &t, nullptr);
  if (rc != VGX_OK) return rc;
  return range_image_box(kTwoPi / (double)model->width, t.ext_max, *image_counts, *cfg, T_G_S, voxel_size, voxels_per_side, lo, hi, nullptr);
}

int vgx_view_rays_lidar_beams(const vgx_lidar_beam_model* model, float* dirs) {
  if (!dirs || beam_model_check(model, nullptr, nullptr) != VGX_OK) return VGX_ERR_INVALID;
  const double su = (model->azimuth_clockwise ? -1.0 : 1.0) * (double)model->width / kTwoPi;
  for (int32_t r = 0; r < model->height; ++r) {
    const double el = (double)model->row_elevation_rad[r];
    const double az0 = (double)model->azimuth_first_rad + (model->row_azimuth_offset_rad ? (double)model->row_azimuth_offset_rad[r] : 0.0);
    for (int32_t c = 0; c < model->width; ++c) {
      const double az = az0 + (double)c / su;
      float* o = dirs + 3 * ((size_t)r * (size_t)model->width + (size_t)c);
      o[0] = (float)(std::cos(el) * std::cos(az));
      o[1] = (float)(std::cos(el) * std::sin(az));
      o[2] = (float)std::sin(el);
    }
  }
  return VGX_OK;
}

}  // extern "C"
