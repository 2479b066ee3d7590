// The elevation map: a layer's height band read as a 2.5D surface -- per cell the height of the zero crossing of its
// column to sub-voxel accuracy, the headroom above it, the step height and support of its neighbourhood, the gradient
// and slope of the surface, a traversability class, and the exact planar Euclidean distance to the nearest obstacle
// cell, clipped.  The formulation is this library's own (nothing in voxgraph or voxblox does it); the rules are stated
// in include/voxgraph_amd.h (vgx_elevation_map), the passes and their measurement in DESIGN.md 35.
//
//   0. planar_box_kernel (default box only): the planar map's, vgx_planar_passes.h
//   1. elevation_gather_kernel: one lane per cell, a workgroup per 16 x 16 cells aligned to the block grid.  A lane walks
//      the band's z blocks through the layer's dense block table in DESCENDING z, carrying the run of free voxels above
//      the current row; adjacent lanes are adjacent in x, so a voxel row is one contiguous read per block row.  No
//      atomics on cells; the four state totals are ballots, LDS integer adds and four integer atomics per workgroup
//   2. elevation_step_row_kernel: min, max and count of the surface heights of row y within the window, the tile and
//      its halo in x held in LDS
//   3. elevation_step_class_kernel: the same down the columns over the row pass's results (tile and halo in y in LDS):
//      step and support; then the gradient, the slope and the class of the cell; the three class totals as in 1
//   4. planar_row_kernel / 5. planar_column_kernel over the class: the planar map's, vgx_planar_passes.h
// A fixed number of launches whatever the size; two host synchronisations (one with a given box); no float atomics.
#include <climits>
#include <cmath>
#include <string>

#include "vgx_cloud_src.h"
#include "vgx_internal.h"
#include "vgx_planar_passes.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

constexpr int kElevationMaxRadius = 64;
constexpr int kElevationRowSpan = kPlanarPassX + 2 * kElevationMaxRadius;  // the row pass's tile and halo, cells

struct ElevationRule {
  float z_min, z_max, min_weight, max_slope, max_step_m, max_distance_m;
  int32_t min_free_voxels, pick, radius, min_support, min_headroom_voxels, hole_is_obstacle, unknown_is_obstacle, R;
  int32_t bz_lo, bz_hi;  // the z blocks of the table with a row in the band lie in [bz_lo, bz_hi] (empty: lo > hi)
};

template <int VPS, int SRC>
__global__ __launch_bounds__(256) void elevation_gather_kernel(CloudSrc s, PlanarTable t, ElevationRule r, PlanarBox b,
                                                               uint8_t* __restrict__ state, float* __restrict__ height,
                                                               int32_t* __restrict__ headroom, uint8_t* __restrict__ crossings,
                                                               unsigned long long* __restrict__ totals) {
  constexpr int SHIFT = VPS == 16 ? 4 : 3;
  constexpr int VOX = VPS * VPS * VPS;
  __shared__ int s_tot[4];
  if (threadIdx.x < 4) s_tot[threadIdx.x] = 0;
  __syncthreads();
  const int tile_x = (int)(blockIdx.x % (unsigned)b.tiles_x), tile_y = (int)(blockIdx.x / (unsigned)b.tiles_x);
  const long long gx = b.tx0 + (long long)kPlanarTile * tile_x + (long long)(threadIdx.x & (kPlanarTile - 1));
  const long long gy = b.ty0 + (long long)kPlanarTile * tile_y + (long long)(threadIdx.x / kPlanarTile);
  const bool inside = gx >= (long long)b.x0 && gx < (long long)b.x0 + b.W && gy >= (long long)b.y0 && gy < (long long)b.y0 + b.H;
  int st = 0;
  if (inside) {
    const int ix = (int)gx, iy = (int)gy;
    const int bx = ix >> SHIFT, by = iy >> SHIFT;  // (arithmetic shifts: floor)
    const int lx = ix & (VPS - 1), ly = iy & (VPS - 1);
    const long long rx = (long long)bx - t.lut_min[0], ry = (long long)by - t.lut_min[1];
    int run = 0, n_free = 0, n_solid = 0, n_cross = 0, head = 0;
    float d_u = 0.0f, h_pick = 0.0f;
    if (rx >= 0 && rx < (long long)t.lut_dim[0] && ry >= 0 && ry < (long long)t.lut_dim[1]) {
      const float vs = s.voxel_size;
      for (int bz = r.bz_hi; bz >= r.bz_lo; --bz) {
        const uint32_t rows = planar_band_rows<VPS>(r.z_min, r.z_max, bz, vs);  // (uniform)
        const size_t rz = (size_t)(bz - t.lut_min[2]);
        const int slot = rows == 0u ? -1 : t.lut[(size_t)rx + (size_t)t.lut_dim[0] * ((size_t)ry + (size_t)t.lut_dim[1] * rz)];
        if (slot < 0 || slot >= t.slots) {  // a missing block's rows, or rows out of the band: nothing is adjacent across them
          run = 0;
          continue;
        }
        const size_t base = (size_t)slot * VOX + (size_t)(lx + VPS * ly);
        const float origin = (float)bz * ((float)VPS * vs);
#pragma unroll
        for (int lz = VPS - 1; lz >= 0; --lz) {
          if (!((rows >> lz) & 1u)) {
            run = 0;
            continue;
          }
          float d;
          const bool seen = cloud_voxel<SRC>(s, base + (size_t)(VPS * VPS * lz), r.min_weight, &d);
          if (seen && d > 0.0f) {  // free_v
            ++n_free;
            ++run;
            d_u = d;
            continue;
          }
          if (seen && d <= 0.0f) {  // solid_v (a NaN is neither)
            ++n_solid;
            if (run >= 1) {  // a crossing between this voxel and the free one directly above it
              float tt = (-d) / (d_u - d);
              if (!(tt >= 0.0f && tt <= 1.0f)) tt = 0.5f;
              if (r.pick == 1 || n_cross == 0) {
                h_pick = voxel_centre(origin, lz, vs) + tt * vs;
                head = run;
              }
              ++n_cross;
            }
          }
          run = 0;
        }
      }
    }
    st = n_cross >= 1 ? 1 : (n_solid >= 1 ? 3 : (n_free >= r.min_free_voxels ? 2 : 0));
    const size_t cell = (size_t)(gy - b.y0) * (size_t)b.W + (size_t)(gx - b.x0);
    state[cell] = (uint8_t)st;
    height[cell] = st == 1 ? h_pick : 0.0f;
    headroom[cell] = st == 1 ? head : 0;
    crossings[cell] = (uint8_t)(n_cross < 255 ? n_cross : 255);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = __popcll(__ballot(inside && st == k));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_tot[k], n);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_tot[threadIdx.x]) atomicAdd(totals + threadIdx.x, (unsigned long long)s_tot[threadIdx.x]);
}

// Row y: the smallest and the largest surface height and the number of surface cells among x - radius .. x + radius inside
// the box (+inf, -inf, 0 where there is none); for every cell, whatever its own state: the column pass combines them.
__global__ __launch_bounds__(256) void elevation_step_row_kernel(const uint8_t* __restrict__ state, const float* __restrict__ height,
                                                                 int W, int H, int tiles_x, int radius, float* __restrict__ row_min,
                                                                 float* __restrict__ row_max, uint16_t* __restrict__ row_count) {
  __shared__ float s_h[kPlanarPassY][kElevationRowSpan];
  __shared__ uint8_t s_on[kPlanarPassY][kElevationRowSpan];
  const int x_tile = kPlanarPassX * (int)(blockIdx.x % (unsigned)tiles_x), y_tile = kPlanarPassY * (int)(blockIdx.x / (unsigned)tiles_x);
  const int span = kPlanarPassX + 2 * radius;
  for (int i = (int)threadIdx.x; i < kPlanarPassY * span; i += 256) {
    const int ry = i / span, rx = i - ry * span;
    const int x = x_tile - radius + rx, y = y_tile + ry;
    bool on = false;
    float h = 0.0f;
    if (x >= 0 && x < W && y < H) {  // the window is cut at the box
      const size_t cell = (size_t)y * (size_t)W + (size_t)x;
      on = state[cell] == 1;
      h = height[cell];
    }
    s_h[ry][rx] = h;
    s_on[ry][rx] = on ? 1 : 0;
  }
  __syncthreads();
  const int tx = (int)(threadIdx.x % kPlanarPassX), ty = (int)(threadIdx.x / kPlanarPassX);
  const int x = x_tile + tx, y = y_tile + ty;
  if (x >= W || y >= H) return;
  float lo = INFINITY, hi = -INFINITY;
  int n = 0;
  for (int k = 0; k <= 2 * radius; ++k) {
    if (!s_on[ty][tx + k]) continue;
    const float h = s_h[ty][tx + k];
    lo = h < lo ? h : lo;
    hi = h > hi ? h : hi;
    ++n;
  }
  const size_t cell = (size_t)y * (size_t)W + (size_t)x;
  row_min[cell] = lo;
  row_max[cell] = hi;
  row_count[cell] = (uint16_t)n;
}

struct ElevationCells {
  const uint8_t* state;
  const float* height;
  const int32_t* headroom;
  const float *row_min, *row_max;
  const uint16_t* row_count;
  uint16_t* support;
  float *step, *grad, *slope;
  uint8_t *slope_valid, *cls;
};

// one axis of the gradient: the neighbours' heights where they are inside the box and on a surface
__device__ __forceinline__ bool elevation_axis(bool left, float h_l, bool right, float h_r, float h, float vs, float* g) {
  if (left && right) *g = (h_r - h_l) / (2.0f * vs);
  else if (right) *g = (h_r - h) / vs;
  else if (left) *g = (h - h_l) / vs;
  else return false;
  return true;
}

// Dynamic LDS: f32 lo [rows][32], f32 hi [rows][32], u16 n [rows][32], rows = 8 + 2 radius.
__global__ __launch_bounds__(256) void elevation_step_class_kernel(ElevationCells c, ElevationRule r, int W, int H, int tiles_x,
                                                                   float voxel_size, unsigned long long* __restrict__ totals) {
  extern __shared__ __align__(16) float s_dyn[];
  __shared__ int s_tot[4];
  const int radius = r.radius, rows = kPlanarPassY + 2 * radius;
  float* s_lo = s_dyn;
  float* s_hi = s_dyn + rows * kPlanarPassX;
  uint16_t* s_n = reinterpret_cast<uint16_t*>(s_dyn + 2 * rows * kPlanarPassX);
  if (threadIdx.x < 4) s_tot[threadIdx.x] = 0;
  const int x_tile = kPlanarPassX * (int)(blockIdx.x % (unsigned)tiles_x), y_tile = kPlanarPassY * (int)(blockIdx.x / (unsigned)tiles_x);
  for (int i = (int)threadIdx.x; i < rows * kPlanarPassX; i += 256) {
    const int ry = i / kPlanarPassX, rx = i - ry * kPlanarPassX;
    const int x = x_tile + rx, y = y_tile - radius + ry;
    float lo = INFINITY, hi = -INFINITY;
    uint16_t n = 0;
    if (x < W && y >= 0 && y < H) {  // the window is cut at the box
      const size_t cell = (size_t)y * (size_t)W + (size_t)x;
      lo = c.row_min[cell];
      hi = c.row_max[cell];
      n = c.row_count[cell];
    }
    s_lo[i] = lo;
    s_hi[i] = hi;
    s_n[i] = n;
  }
  __syncthreads();
  const int tx = (int)(threadIdx.x % kPlanarPassX), ty = (int)(threadIdx.x / kPlanarPassX);
  const int x = x_tile + tx, y = y_tile + ty;
  const bool inside = x < W && y < H;
  int cls = 0;
  if (inside) {
    const size_t cell = (size_t)y * (size_t)W + (size_t)x;
    const int st = c.state[cell];
    int support = 0;
    float step = 0.0f, gx = 0.0f, gy = 0.0f, slope = 0.0f;
    bool valid = false;
    if (st == 1) {
      float lo = INFINITY, hi = -INFINITY;
      for (int k = 0; k <= 2 * radius; ++k) {
        const int at = (ty + k) * kPlanarPassX + tx;
        const float a = s_lo[at], z = s_hi[at];
        lo = a < lo ? a : lo;
        hi = z > hi ? z : hi;
        support += s_n[at];
      }
      step = hi - lo;  // (the cell itself is in its window: both are finite)
      const float h = c.height[cell];
      const bool xl = x > 0 && c.state[cell - 1] == 1, xr = x + 1 < W && c.state[cell + 1] == 1;
      const bool yl = y > 0 && c.state[cell - (size_t)W] == 1, yr = y + 1 < H && c.state[cell + (size_t)W] == 1;
      const bool has_x = elevation_axis(xl, xl ? c.height[cell - 1] : 0.0f, xr, xr ? c.height[cell + 1] : 0.0f, h, voxel_size, &gx);
      const bool has_y = elevation_axis(yl, yl ? c.height[cell - (size_t)W] : 0.0f, yr, yr ? c.height[cell + (size_t)W] : 0.0f, h,
                                        voxel_size, &gy);
      valid = has_x && has_y;
      if (valid) {
        slope = sqrtf(gx * gx + gy * gy);
      } else {
        gx = gy = 0.0f;
      }
      if (c.headroom[cell] < r.min_headroom_voxels) cls = 2;
      else if (!valid || support < r.min_support) cls = 0;
      else if (slope > r.max_slope || step > r.max_step_m) cls = 2;
      else cls = 1;
    } else if (st == 3) {
      cls = 2;
    } else if (st == 2) {
      cls = r.hole_is_obstacle != 0 ? 2 : 0;
    }
    c.support[cell] = (uint16_t)support;
    c.step[cell] = step;
    c.grad[2 * cell] = gx;
    c.grad[2 * cell + 1] = gy;
    c.slope[cell] = slope;
    c.slope_valid[cell] = valid ? 1 : 0;
    c.cls[cell] = (uint8_t)cls;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int n = __popcll(__ballot(inside && cls == k));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_tot[k], n);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(totals + threadIdx.x, (unsigned long long)s_tot[threadIdx.x]);
}

}  // namespace vgx

using namespace vgx;

struct vgx_elevation_map_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  // the map held now
  int32_t x0 = 0, y0 = 0, W = 0, H = 0;
  float voxel_size = 0.0f;
  int64_t state_counts[4] = {0, 0, 0, 0};
  int64_t class_counts[3] = {0, 0, 0};
  // grown on demand to exactly what a map needs, together
  size_t cap_cells = 0;
  DeviceBuffer d_state;        // u8 [H][W]
  DeviceBuffer d_height;       // f32 [H][W]
  DeviceBuffer d_headroom;     // i32 [H][W]
  DeviceBuffer d_crossings;    // u8 [H][W]
  DeviceBuffer d_support;      // u16 [H][W]
  DeviceBuffer d_step;         // f32 [H][W]
  DeviceBuffer d_grad;         // f32 [H][W][2]
  DeviceBuffer d_slope;        // f32 [H][W]
  DeviceBuffer d_slope_valid;  // u8 [H][W]
  DeviceBuffer d_class;        // u8 [H][W]
  DeviceBuffer d_distance;     // f32 [H][W]
  DeviceBuffer d_row_min, d_row_max, d_row_count;  // f32, f32, u16 [H][W]: the step row pass
  DeviceBuffer d_g;                                // u16 [H][W]: the distance row pass
  DeviceBuffer d_meta;                             // u64 state totals[4] at 0, u64 class totals[3] at 32, i32 box[4] at 64
  // vgx_elevation_map_set_timing: the last producing call by pass, from events either side of the box kernel (0, 1),
  // before the gather (2) and after each of the five passes (3 .. 7); made at the first timed call.  Off (the default):
  // no event is made or recorded
  bool timing = false;
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float pass_ms[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // box, gather, step row, step column + class, distance row, column
  ~vgx_elevation_map_s() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// Refusals shared by the two producers, before anything is written; the rule comes back without its z blocks.
int elevation_check(vgx_ctx ctx, const char* fn, const vgx_elevation_map_config* cfg, vgx_elevation_map M, float voxel_size,
                    ElevationRule* rule) {
  auto fail = [ctx, fn](const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": " + msg); };
  if (!M) return fail("NULL map");
  if (M->ctx != ctx) return fail("the map belongs to another context");
  if (!cfg) return fail("NULL config (there is no default band)");
  const vgx_elevation_map_config& c = *cfg;
  if (!std::isfinite(c.z_min) || !std::isfinite(c.z_max)) return fail("z_min or z_max is not finite (the band must be set)");
  if (c.z_min > c.z_max) return fail("z_min > z_max");
  if (!std::isfinite(c.min_weight) || c.min_weight < 0.0f) return fail("min_weight is negative or not finite");
  if (c.min_free_voxels < 1) return fail("min_free_voxels < 1");
  if (c.pick != 0 && c.pick != 1) return fail("pick is neither 0 (highest) nor 1 (lowest)");
  if (c.step_radius_cells < 0 || c.step_radius_cells > kElevationMaxRadius) return fail("step_radius_cells outside 0..64");
  if (c.min_support < 1) return fail("min_support < 1");
  if (c.min_headroom_voxels < 1) return fail("min_headroom_voxels < 1");
  if (std::isnan(c.max_slope) || c.max_slope < 0.0f) return fail("max_slope is negative or NaN");
  if (std::isnan(c.max_step_m) || c.max_step_m < 0.0f) return fail("max_step_m is negative or NaN");
  if (!std::isfinite(c.max_distance_m) || !(c.max_distance_m > 0.0f)) return fail("max_distance_m is not finite and positive");
  const double cells = std::ceil((double)c.max_distance_m / (double)voxel_size);
  if (!(cells <= (double)kPlanarMaxR)) return fail("max_distance_m is more than 2048 voxels");
  if (c.use_box != 0) {
    if (c.cell_dim[0] < 0 || c.cell_dim[1] < 0) return fail("a negative cell_dim");
    for (int a = 0; a < 2; ++a)
      if ((long long)c.cell_min[a] + (long long)c.cell_dim[a] > (long long)INT32_MAX) return fail("cell_min + cell_dim overflows int32");
    if ((long long)c.cell_dim[0] * (long long)c.cell_dim[1] > kPlanarMaxCells) return fail("a box of more than 2^28 cells");
  }
  *rule = ElevationRule{c.z_min, c.z_max, c.min_weight, c.max_slope, c.max_step_m, c.max_distance_m, c.min_free_voxels, c.pick,
                        c.step_radius_cells, c.min_support, c.min_headroom_voxels, c.hole_is_obstacle, c.unknown_is_obstacle,
                        (int32_t)cells, 0, -1};
  return VGX_OK;
}

int ensure_cells(vgx_elevation_map M, size_t n) {
  if (!M->d_meta.p) {
    const hipError_t e = M->d_meta.alloc(128);
    if (e != hipSuccess) return alloc_error(M->ctx, e, "elevation map: allocating totals");
  }
  if (n <= M->cap_cells) return VGX_OK;
  M->cap_cells = 0;
  const hipError_t e = alloc_group({{&M->d_state, n}, {&M->d_height, n * 4}, {&M->d_headroom, n * 4}, {&M->d_crossings, n},
                                    {&M->d_support, n * 2}, {&M->d_step, n * 4}, {&M->d_grad, n * 8}, {&M->d_slope, n * 4},
                                    {&M->d_slope_valid, n}, {&M->d_class, n}, {&M->d_distance, n * 4}, {&M->d_row_min, n * 4},
                                    {&M->d_row_max, n * 4}, {&M->d_row_count, n * 2}, {&M->d_g, n * 2}});
  if (e != hipSuccess) return alloc_error(M->ctx, e, "elevation map: allocating cells");
  M->cap_cells = n;
  return VGX_OK;
}

template <int VPS, int SRC>
void launch_gather(hipStream_t st, const CloudSrc& s, const PlanarTable& t, const ElevationRule& r, const PlanarBox& b, vgx_elevation_map M) {
  hipLaunchKernelGGL((elevation_gather_kernel<VPS, SRC>), dim3((unsigned)b.tiles_x * (unsigned)b.tiles_y), dim3(256), 0, st, s, t, r, b,
                     M->d_state.as<uint8_t>(), M->d_height.as<float>(), M->d_headroom.as<int32_t>(), M->d_crossings.as<uint8_t>(),
                     M->d_meta.as<unsigned long long>());
}

void clear_pass_ms(vgx_elevation_map M) {
  for (float& v : M->pass_ms) v = 0.0f;
}

// The passes on stream st (the caller holds the map's and the stream's locks, the device is set).  `slots`: block slots
// of the pool; s.live_blocks says how many of them are blocks where only the device knows.
int elevation_generate(vgx_ctx ctx, const char* fn, hipStream_t st, int src, int vps, const CloudSrc& s, const PlanarTable& t,
                       ElevationRule r, const vgx_elevation_map_config& cfg, int slots, vgx_elevation_map M) {
  planar_band_blocks(t, vps, r.z_min, r.z_max, s.voxel_size, &r.bz_lo, &r.bz_hi);
  if (!M->d_meta.p) {
    const int rc = ensure_cells(M, 0);
    if (rc != VGX_OK) return rc;
  }
  const bool timing = M->timing;
  if (timing)
    for (hipEvent_t& e : M->ev)
      if (!e) VGX_HIP(ctx, hipEventCreate(&e));
  bool boxed = false;
  unsigned long long* d_totals = M->d_meta.as<unsigned long long>();
  int32_t* d_box = reinterpret_cast<int32_t*>(static_cast<char*>(M->d_meta.p) + 64);
  long long box[4];
  int rc = planar_find_box(ctx, fn, st, vps, s, r.z_min, r.z_max, r.bz_lo <= r.bz_hi, slots, cfg.use_box, cfg.cell_min, cfg.cell_dim, d_box,
                           timing ? M->ev : nullptr, box, &boxed);
  if (rc != VGX_OK) return rc;
  boxed = boxed && timing;
  const long long x0 = box[0], y0 = box[1], W = box[2], H = box[3];
  const size_t cells = (size_t)(W * H);
  // from here on the map is replaced
  M->W = M->H = 0;
  for (int64_t& v : M->state_counts) v = 0;
  for (int64_t& v : M->class_counts) v = 0;
  clear_pass_ms(M);
  rc = ensure_cells(M, cells);
  if (rc != VGX_OK) return rc;
  unsigned long long totals[7] = {0, 0, 0, 0, 0, 0, 0};
  if (cells > 0) {
    const PlanarBox b = planar_make_box(x0, y0, W, H);
    VGX_HIP(ctx, hipMemsetAsync(d_totals, 0, 56, st));
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[2], st));
    if (vps == 16) {
      if (src == kCloudSrcEsdf) launch_gather<16, kCloudSrcEsdf>(st, s, t, r, b, M);
      else if (src == kCloudSrcTsdf) launch_gather<16, kCloudSrcTsdf>(st, s, t, r, b, M);
      else launch_gather<16, kCloudSrcPacked>(st, s, t, r, b, M);
    } else {
      if (src == kCloudSrcEsdf) launch_gather<8, kCloudSrcEsdf>(st, s, t, r, b, M);
      else if (src == kCloudSrcTsdf) launch_gather<8, kCloudSrcTsdf>(st, s, t, r, b, M);
      else launch_gather<8, kCloudSrcPacked>(st, s, t, r, b, M);
    }
    VGX_HIP(ctx, hipGetLastError());
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[3], st));
    const int ptx = (int)((W + kPlanarPassX - 1) / kPlanarPassX), pty = (int)((H + kPlanarPassY - 1) / kPlanarPassY);
    const dim3 grid((unsigned)ptx * (unsigned)pty);
    hipLaunchKernelGGL(elevation_step_row_kernel, grid, dim3(256), 0, st, M->d_state.as<uint8_t>(), M->d_height.as<float>(), (int)W, (int)H,
                       ptx, r.radius, M->d_row_min.as<float>(), M->d_row_max.as<float>(), M->d_row_count.as<uint16_t>());
    VGX_HIP(ctx, hipGetLastError());
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[4], st));
    const ElevationCells c{M->d_state.as<uint8_t>(),   M->d_height.as<float>(),     M->d_headroom.as<int32_t>(), M->d_row_min.as<float>(),
                           M->d_row_max.as<float>(),   M->d_row_count.as<uint16_t>(), M->d_support.as<uint16_t>(), M->d_step.as<float>(),
                           M->d_grad.as<float>(),      M->d_slope.as<float>(),      M->d_slope_valid.as<uint8_t>(), M->d_class.as<uint8_t>()};
    const size_t lds = (size_t)(kPlanarPassY + 2 * r.radius) * kPlanarPassX * 10;  // at most 43520 bytes (radius 64)
    hipLaunchKernelGGL(elevation_step_class_kernel, grid, dim3(256), lds, st, c, r, (int)W, (int)H, ptx, s.voxel_size, d_totals + 4);
    VGX_HIP(ctx, hipGetLastError());
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[5], st));
    hipLaunchKernelGGL(planar_row_kernel<PlanarObstacle>, grid, dim3(256), 0, st, M->d_class.as<uint8_t>(), (int)W, (int)H, ptx, r.R,
                       PlanarObstacle{r.unknown_is_obstacle}, M->d_g.as<uint16_t>());
    VGX_HIP(ctx, hipGetLastError());
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[6], st));
    hipLaunchKernelGGL(planar_column_kernel, grid, dim3(256), 0, st, M->d_g.as<uint16_t>(), (int)W, (int)H, ptx, r.R, s.voxel_size,
                       r.max_distance_m, M->d_distance.as<float>());
    VGX_HIP(ctx, hipGetLastError());
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[7], st));
    VGX_HIP(ctx, hipMemcpyAsync(totals, d_totals, 56, hipMemcpyDeviceToHost, st));
    VGX_HIP(ctx, hipStreamSynchronize(st));
    for (int k = 0; k < 5 && timing; ++k) VGX_HIP(ctx, hipEventElapsedTime(&M->pass_ms[1 + k], M->ev[2 + k], M->ev[3 + k]));
  }
  if (boxed) VGX_HIP(ctx, hipEventElapsedTime(&M->pass_ms[0], M->ev[0], M->ev[1]));
  M->x0 = (int32_t)x0;
  M->y0 = (int32_t)y0;
  M->W = (int32_t)W;
  M->H = (int32_t)H;
  M->voxel_size = s.voxel_size;
  for (int k = 0; k < 4; ++k) M->state_counts[k] = (int64_t)totals[k];
  for (int k = 0; k < 3; ++k) M->class_counts[k] = (int64_t)totals[4 + k];
  return VGX_OK;
}

}  // namespace

extern "C" {

void vgx_elevation_map_config_default(vgx_elevation_map_config* cfg) {
  if (!cfg) return;
  cfg->z_min = cfg->z_max = std::nanf("");
  cfg->min_weight = 1e-3f;
  cfg->min_free_voxels = 1;
  cfg->pick = 0;
  cfg->step_radius_cells = 1;
  cfg->min_support = 1;
  cfg->max_slope = 1.0f;
  cfg->max_step_m = 0.2f;
  cfg->min_headroom_voxels = 1;
  cfg->hole_is_obstacle = 1;
  cfg->unknown_is_obstacle = 0;
  cfg->max_distance_m = 2.0f;
  cfg->use_box = 0;
  cfg->cell_min[0] = cfg->cell_min[1] = 0;
  cfg->cell_dim[0] = cfg->cell_dim[1] = 0;
}

int vgx_elevation_map_create(vgx_ctx ctx, vgx_elevation_map* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_elevation_map_create: NULL argument");
  vgx_elevation_map M = new vgx_elevation_map_s;
  M->ctx = ctx;
  *out = M;
  return VGX_OK;
}

int vgx_elevation_map_destroy(vgx_elevation_map M) {
  if (!M) return VGX_ERR_INVALID;
  (void)hipSetDevice(M->ctx->device);
  delete M;
  return VGX_OK;
}

int vgx_elevation_map_stats(vgx_elevation_map M, int32_t cell_min[2], int32_t cell_dim[2], float* voxel_size, int64_t state_counts[4],
                            int64_t class_counts[3]) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  if (cell_min) {
    cell_min[0] = M->x0;
    cell_min[1] = M->y0;
  }
  if (cell_dim) {
    cell_dim[0] = M->W;
    cell_dim[1] = M->H;
  }
  if (voxel_size) *voxel_size = M->voxel_size;
  if (state_counts)
    for (int k = 0; k < 4; ++k) state_counts[k] = M->state_counts[k];
  if (class_counts)
    for (int k = 0; k < 3; ++k) class_counts[k] = M->class_counts[k];
  return VGX_OK;
}

int vgx_elevation_map_set_timing(vgx_elevation_map M, int32_t enable) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  M->timing = enable != 0;
  if (!M->timing) clear_pass_ms(M);
  return VGX_OK;
}

int vgx_elevation_map_pass_ms(vgx_elevation_map M, float ms[6]) {
  if (!M || !ms) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  for (int k = 0; k < 6; ++k) ms[k] = M->pass_ms[k];
  return VGX_OK;
}

int vgx_elevation_map_device_pointers(vgx_elevation_map M, const uint8_t** state, const float** height, const int32_t** headroom,
                                      const uint8_t** crossings, const uint16_t** support, const float** step, const float** grad,
                                      const float** slope, const uint8_t** slope_valid, const uint8_t** cls, const float** distance) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  const bool any = (size_t)M->W * (size_t)M->H > 0;
  if (state) *state = any ? M->d_state.as<uint8_t>() : nullptr;
  if (height) *height = any ? M->d_height.as<float>() : nullptr;
  if (headroom) *headroom = any ? M->d_headroom.as<int32_t>() : nullptr;
  if (crossings) *crossings = any ? M->d_crossings.as<uint8_t>() : nullptr;
  if (support) *support = any ? M->d_support.as<uint16_t>() : nullptr;
  if (step) *step = any ? M->d_step.as<float>() : nullptr;
  if (grad) *grad = any ? M->d_grad.as<float>() : nullptr;
  if (slope) *slope = any ? M->d_slope.as<float>() : nullptr;
  if (slope_valid) *slope_valid = any ? M->d_slope_valid.as<uint8_t>() : nullptr;
  if (cls) *cls = any ? M->d_class.as<uint8_t>() : nullptr;
  if (distance) *distance = any ? M->d_distance.as<float>() : nullptr;
  return VGX_OK;
}

int vgx_elevation_map_download(vgx_elevation_map M, uint8_t* state, float* height, int32_t* headroom, uint8_t* crossings, uint16_t* support,
                               float* step, float* grad, float* slope, uint8_t* slope_valid, uint8_t* cls, float* distance) {
  if (!M) return VGX_ERR_INVALID;
  vgx_ctx ctx = M->ctx;
  std::lock_guard<std::mutex> lk(M->mu);
  const size_t n = (size_t)M->W * (size_t)M->H;
  if (n == 0) return VGX_OK;
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the map was complete when its producer returned, whichever stream made it)
  const struct {
    void* to;
    const DeviceBuffer* from;
    size_t bytes;
  } copies[] = {{state, &M->d_state, n},       {height, &M->d_height, n * 4}, {headroom, &M->d_headroom, n * 4},
                {crossings, &M->d_crossings, n}, {support, &M->d_support, n * 2}, {step, &M->d_step, n * 4},
                {grad, &M->d_grad, n * 8},     {slope, &M->d_slope, n * 4},   {slope_valid, &M->d_slope_valid, n},
                {cls, &M->d_class, n},         {distance, &M->d_distance, n * 4}};
  for (const auto& c : copies)
    if (c.to) VGX_HIP(ctx, hipMemcpyAsync(c.to, c.from->p, c.bytes, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  return VGX_OK;
}

int vgx_submap_layer_elevation_map(vgx_submap sm, int32_t layer, const vgx_elevation_map_config* cfg, vgx_elevation_map M) {
  static const char* kFn = "vgx_submap_layer_elevation_map";
  if (!sm) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL submap");
  vgx_ctx ctx = sm->ctx;
  ElevationRule rule{};
  int rc = elevation_check(ctx, kFn, cfg, M, sm->voxel_size, &rule);
  if (rc != VGX_OK) return rc;
  if (layer != VGX_EVAL_LAYER_ESDF && layer != VGX_EVAL_LAYER_TSDF)
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": layer is neither ESDF nor TSDF");
  const bool tsdf = layer == VGX_EVAL_LAYER_TSDF;
  // the submap's layers and block table are read under the registration lock: another thread may release or generate them
  std::lock_guard<std::mutex> map_lk(M->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  CloudSrc s{};
  PlanarTable t{};
  rc = planar_submap_source(sm, tsdf, kFn, &s, &t);
  if (rc != VGX_OK) return rc;
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  return elevation_generate(ctx, kFn, ctx->stream, tsdf ? kCloudSrcTsdf : kCloudSrcEsdf, sm->vps, s, t, rule, *cfg, sm->n_blocks, M);
}

int vgx_tsdf_layer_elevation_map(vgx_tsdf_layer L, const vgx_elevation_map_config* cfg, vgx_elevation_map M) {
  static const char* kFn = "vgx_tsdf_layer_elevation_map";
  if (!L) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL layer");
  vgx_ctx ctx = L->ctx;
  ElevationRule rule{};
  int rc = elevation_check(ctx, kFn, cfg, M, L->dev.voxel_size, &rule);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> map_lk(M->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  CloudSrc s{};
  PlanarTable t{};
  rc = planar_layer_source(L, kFn, &s, &t);
  if (rc != VGX_OK) return rc;
  const TsdfLayerDev& d = L->dev;
  return elevation_generate(ctx, kFn, ctx->tsdf_stream, kCloudSrcPacked, d.vps, s, t, rule, *cfg, d.max_blocks, M);
}

}  // extern "C"
