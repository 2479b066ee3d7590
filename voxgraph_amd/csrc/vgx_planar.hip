// The planar map: a layer's height band collapsed along z into a 2D grid -- state, nav_msgs/OccupancyGrid occupancy,
// clearance, obstacle height -- and the exact planar Euclidean distance to the nearest obstacle cell, clipped.  The rules
// are stated in include/voxgraph_amd.h (vgx_planar_map), the passes and their measurement in DESIGN.md 34.
//
//   0. planar_box_kernel (default box only): one thread per block slot; the x/y extent of the blocks with a row in the
//      band, by integer atomicMin after a wave reduction; it comes back in the first of the two synchronisations
//   1. planar_gather_kernel: one lane per cell, a workgroup per 16 x 16 cells aligned to the block grid (one block column
//      at vps 16, four at vps 8).  A lane walks the band's z blocks through the layer's dense block table in ascending z;
//      adjacent lanes are adjacent in x, so a voxel row is one contiguous read per block row.  No atomics on cells; the
//      three totals are ballots, LDS integer adds and three integer atomics per workgroup
//   2. planar_row_kernel: g[y][x] = the distance in cells to the nearest obstacle cell of row y within R, or none (u16)
//   3. planar_column_kernel: d2 = min over |dy| <= R of dy^2 + g[y + dy][x]^2 (int), left once dy^2 >= the best so far;
//      then sqrtf, the voxel size and the clip
// A fixed number of launches whatever the size.  The source layouts are those of the layer clouds (vgx_cloud_src.h); the
// box kernel and the two distance passes are shared with the elevation map (vgx_planar_passes.h).
#include <climits>
#include <cmath>
#include <string>

#include "vgx_cloud_src.h"
#include "vgx_internal.h"
#include "vgx_planar_passes.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

struct PlanarRule {
  float z_min, z_max, occupied_distance, min_weight, max_distance_m;
  int32_t min_free_voxels, unknown_is_obstacle, R;
  int32_t bz_lo, bz_hi;  // the z blocks of the table with a row in the band lie in [bz_lo, bz_hi] (empty: lo > hi)
};

template <int VPS, int SRC>
__global__ __launch_bounds__(256) void planar_gather_kernel(CloudSrc s, PlanarTable t, PlanarRule r, PlanarBox b,
                                                            uint8_t* __restrict__ state, int8_t* __restrict__ occupancy,
                                                            float* __restrict__ clearance, float* __restrict__ height,
                                                            unsigned long long* __restrict__ totals) {
  constexpr int SHIFT = VPS == 16 ? 4 : 3;
  constexpr int VOX = VPS * VPS * VPS;
  __shared__ int s_tot[3];
  if (threadIdx.x < 3) s_tot[threadIdx.x] = 0;
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
    int n_occ = 0, n_free = 0;
    bool any = false;
    float best = 0.0f, top = 0.0f;
    if (rx >= 0 && rx < (long long)t.lut_dim[0] && ry >= 0 && ry < (long long)t.lut_dim[1]) {
      const float vs = s.voxel_size;
      for (int bz = r.bz_lo; bz <= r.bz_hi; ++bz) {
        const uint32_t rows = planar_band_rows<VPS>(r.z_min, r.z_max, bz, vs);  // (uniform)
        if (rows == 0u) continue;
        const size_t rz = (size_t)(bz - t.lut_min[2]);
        const int slot = t.lut[(size_t)rx + (size_t)t.lut_dim[0] * ((size_t)ry + (size_t)t.lut_dim[1] * rz)];
        if (slot < 0 || slot >= t.slots) continue;
        const size_t base = (size_t)slot * VOX + (size_t)(lx + VPS * ly);
        const float origin = (float)bz * ((float)VPS * vs);
#pragma unroll
        for (int lz = 0; lz < VPS; ++lz) {
          if (!((rows >> lz) & 1u)) continue;
          float d;
          if (!cloud_voxel<SRC>(s, base + (size_t)(VPS * VPS * lz), r.min_weight, &d)) continue;
          const bool occupied_v = d <= r.occupied_distance, free_v = d > r.occupied_distance;
          if (!occupied_v && !free_v) continue;  // NaN
          if (!any || d < best) best = d;
          any = true;
          if (occupied_v) {
            ++n_occ;
            top = voxel_centre(origin, lz, vs);
          } else {
            ++n_free;
          }
        }
      }
    }
    st = n_occ >= 1 ? 2 : (n_free >= r.min_free_voxels ? 1 : 0);
    const size_t cell = (size_t)(gy - b.y0) * (size_t)b.W + (size_t)(gx - b.x0);
    state[cell] = (uint8_t)st;
    occupancy[cell] = st == 2 ? (int8_t)100 : (st == 1 ? (int8_t)0 : (int8_t)-1);
    clearance[cell] = st != 0 ? best : 0.0f;
    height[cell] = st == 2 ? top : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int n = __popcll(__ballot(inside && st == k));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_tot[k], n);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_tot[threadIdx.x]) atomicAdd(totals + threadIdx.x, (unsigned long long)s_tot[threadIdx.x]);
}

}  // namespace vgx

using namespace vgx;

struct vgx_planar_map_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  // the map held now
  int32_t x0 = 0, y0 = 0, W = 0, H = 0;
  float voxel_size = 0.0f;
  int64_t counts[3] = {0, 0, 0};
  // grown on demand to exactly what a map needs, together
  size_t cap_cells = 0;
  DeviceBuffer d_state;      // u8 [H][W]
  DeviceBuffer d_occupancy;  // i8 [H][W]
  DeviceBuffer d_clearance;  // f32 [H][W]
  DeviceBuffer d_height;     // f32 [H][W]
  DeviceBuffer d_distance;   // f32 [H][W]
  DeviceBuffer d_g;          // u16 [H][W]: the row pass
  DeviceBuffer d_meta;       // u64 totals[3] at 0, i32 box[4] at 32
  // vgx_planar_map_set_timing: the last producing call by pass, from events either side of the box kernel (0, 1), before
  // the gather (2) and after the gather, the row pass and the column pass (3, 4, 5); made at the first timed call.  Off
  // (the default): no event is made or recorded
  bool timing = false;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float pass_ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // box, gather, row, column
  ~vgx_planar_map_s() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace {

// Refusals shared by the two producers, before anything is written; the rule comes back without its z blocks.
int planar_check(vgx_ctx ctx, const char* fn, const vgx_planar_map_config* cfg, vgx_planar_map M, float voxel_size, PlanarRule* rule) {
  auto fail = [ctx, fn](const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": " + msg); };
  if (!M) return fail("NULL map");
  if (M->ctx != ctx) return fail("the map belongs to another context");
  if (!cfg) return fail("NULL config (there is no default band)");
  const vgx_planar_map_config& c = *cfg;
  if (!std::isfinite(c.z_min) || !std::isfinite(c.z_max)) return fail("z_min or z_max is not finite (the band must be set)");
  if (c.z_min > c.z_max) return fail("z_min > z_max");
  if (!std::isfinite(c.occupied_distance)) return fail("occupied_distance is not finite");
  if (!std::isfinite(c.min_weight) || c.min_weight < 0.0f) return fail("min_weight is negative or not finite");
  if (c.min_free_voxels < 1) return fail("min_free_voxels < 1");
  if (!std::isfinite(c.max_distance_m) || !(c.max_distance_m > 0.0f)) return fail("max_distance_m is not finite and positive");
  const double cells = std::ceil((double)c.max_distance_m / (double)voxel_size);
  if (!(cells <= (double)kPlanarMaxR)) return fail("max_distance_m is more than 2048 voxels");
  if (c.use_box != 0) {
    if (c.cell_dim[0] < 0 || c.cell_dim[1] < 0) return fail("a negative cell_dim");
    for (int a = 0; a < 2; ++a)
      if ((long long)c.cell_min[a] + (long long)c.cell_dim[a] > (long long)INT32_MAX) return fail("cell_min + cell_dim overflows int32");
    if ((long long)c.cell_dim[0] * (long long)c.cell_dim[1] > kPlanarMaxCells) return fail("a box of more than 2^28 cells");
  }
  *rule = PlanarRule{c.z_min, c.z_max, c.occupied_distance, c.min_weight, c.max_distance_m, c.min_free_voxels, c.unknown_is_obstacle,
                     (int32_t)cells, 0, -1};
  return VGX_OK;
}

int ensure_cells(vgx_planar_map M, size_t n) {
  if (!M->d_meta.p) {
    const hipError_t e = M->d_meta.alloc(64);
    if (e != hipSuccess) return alloc_error(M->ctx, e, "planar map: allocating totals");
  }
  if (n <= M->cap_cells) return VGX_OK;
  M->cap_cells = 0;
  const hipError_t e = alloc_group({{&M->d_state, n}, {&M->d_occupancy, n}, {&M->d_clearance, n * 4}, {&M->d_height, n * 4},
                                    {&M->d_distance, n * 4}, {&M->d_g, n * 2}});
  if (e != hipSuccess) return alloc_error(M->ctx, e, "planar map: allocating cells");
  M->cap_cells = n;
  return VGX_OK;
}

template <int VPS, int SRC>
void launch_gather(hipStream_t st, const CloudSrc& s, const PlanarTable& t, const PlanarRule& r, const PlanarBox& b, vgx_planar_map M) {
  hipLaunchKernelGGL((planar_gather_kernel<VPS, SRC>), dim3((unsigned)b.tiles_x * (unsigned)b.tiles_y), dim3(256), 0, st, s, t, r, b,
                     M->d_state.as<uint8_t>(), M->d_occupancy.as<int8_t>(), M->d_clearance.as<float>(), M->d_height.as<float>(),
                     M->d_meta.as<unsigned long long>());
}

// The passes on stream st (the caller holds the map's and the stream's locks, the device is set).  `slots`: block slots
// of the pool; s.live_blocks says how many of them are blocks where only the device knows.
int planar_generate(vgx_ctx ctx, const char* fn, hipStream_t st, int src, int vps, const CloudSrc& s, const PlanarTable& t,
                    PlanarRule r, const vgx_planar_map_config& cfg, int slots, vgx_planar_map M) {
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
  int32_t* d_box = reinterpret_cast<int32_t*>(static_cast<char*>(M->d_meta.p) + 32);
  long long box[4];
  int rc = planar_find_box(ctx, fn, st, vps, s, r.z_min, r.z_max, r.bz_lo <= r.bz_hi, slots, cfg.use_box, cfg.cell_min, cfg.cell_dim, d_box,
                           timing ? M->ev : nullptr, box, &boxed);
  if (rc != VGX_OK) return rc;
  boxed = boxed && timing;
  const long long x0 = box[0], y0 = box[1], W = box[2], H = box[3];
  const size_t cells = (size_t)(W * H);
  // from here on the map is replaced
  M->W = M->H = 0;
  M->counts[0] = M->counts[1] = M->counts[2] = 0;
  M->pass_ms[0] = M->pass_ms[1] = M->pass_ms[2] = M->pass_ms[3] = 0.0f;
  rc = ensure_cells(M, cells);
  if (rc != VGX_OK) return rc;
  unsigned long long totals[3] = {0, 0, 0};
  if (cells > 0) {
    const PlanarBox b = planar_make_box(x0, y0, W, H);
    VGX_HIP(ctx, hipMemsetAsync(d_totals, 0, 24, st));
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
    hipLaunchKernelGGL(planar_row_kernel<PlanarObstacle>, grid, dim3(256), 0, st, M->d_state.as<uint8_t>(), (int)W, (int)H, ptx, r.R,
                       PlanarObstacle{r.unknown_is_obstacle},
                       M->d_g.as<uint16_t>());
    VGX_HIP(ctx, hipGetLastError());
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[4], st));
    hipLaunchKernelGGL(planar_column_kernel, grid, dim3(256), 0, st, M->d_g.as<uint16_t>(), (int)W, (int)H, ptx, r.R, s.voxel_size,
                       r.max_distance_m, M->d_distance.as<float>());
    VGX_HIP(ctx, hipGetLastError());
    if (timing) VGX_HIP(ctx, hipEventRecord(M->ev[5], st));
    VGX_HIP(ctx, hipMemcpyAsync(totals, d_totals, 24, hipMemcpyDeviceToHost, st));
    VGX_HIP(ctx, hipStreamSynchronize(st));
    for (int k = 0; k < 3 && timing; ++k) VGX_HIP(ctx, hipEventElapsedTime(&M->pass_ms[1 + k], M->ev[2 + k], M->ev[3 + k]));
  }
  if (boxed) VGX_HIP(ctx, hipEventElapsedTime(&M->pass_ms[0], M->ev[0], M->ev[1]));
  M->x0 = (int32_t)x0;
  M->y0 = (int32_t)y0;
  M->W = (int32_t)W;
  M->H = (int32_t)H;
  M->voxel_size = s.voxel_size;
  for (int k = 0; k < 3; ++k) M->counts[k] = (int64_t)totals[k];
  return VGX_OK;
}

}  // namespace

extern "C" {

void vgx_planar_map_config_default(vgx_planar_map_config* cfg) {
  if (!cfg) return;
  cfg->z_min = cfg->z_max = std::nanf("");
  cfg->occupied_distance = 0.0f;
  cfg->min_weight = 1e-3f;
  cfg->min_free_voxels = 1;
  cfg->unknown_is_obstacle = 0;
  cfg->max_distance_m = 2.0f;
  cfg->use_box = 0;
  cfg->cell_min[0] = cfg->cell_min[1] = 0;
  cfg->cell_dim[0] = cfg->cell_dim[1] = 0;
}

int vgx_planar_map_create(vgx_ctx ctx, vgx_planar_map* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_planar_map_create: NULL argument");
  vgx_planar_map M = new vgx_planar_map_s;
  M->ctx = ctx;
  *out = M;
  return VGX_OK;
}

int vgx_planar_map_destroy(vgx_planar_map M) {
  if (!M) return VGX_ERR_INVALID;
  (void)hipSetDevice(M->ctx->device);
  delete M;
  return VGX_OK;
}

int vgx_planar_map_stats(vgx_planar_map M, int32_t cell_min[2], int32_t cell_dim[2], float* voxel_size, int64_t counts[3]) {
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
  if (counts)
    for (int k = 0; k < 3; ++k) counts[k] = M->counts[k];
  return VGX_OK;
}

int vgx_planar_map_set_timing(vgx_planar_map M, int32_t enable) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  M->timing = enable != 0;
  if (!M->timing) M->pass_ms[0] = M->pass_ms[1] = M->pass_ms[2] = M->pass_ms[3] = 0.0f;
  return VGX_OK;
}

int vgx_planar_map_pass_ms(vgx_planar_map M, float ms[4]) {
  if (!M || !ms) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  for (int k = 0; k < 4; ++k) ms[k] = M->pass_ms[k];
  return VGX_OK;
}

int vgx_planar_map_device_pointers(vgx_planar_map M, const uint8_t** state, const int8_t** occupancy, const float** clearance,
                                   const float** height, const float** distance) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  const bool any = (size_t)M->W * (size_t)M->H > 0;
  if (state) *state = any ? M->d_state.as<uint8_t>() : nullptr;
  if (occupancy) *occupancy = any ? M->d_occupancy.as<int8_t>() : nullptr;
  if (clearance) *clearance = any ? M->d_clearance.as<float>() : nullptr;
  if (height) *height = any ? M->d_height.as<float>() : nullptr;
  if (distance) *distance = any ? M->d_distance.as<float>() : nullptr;
  return VGX_OK;
}

int vgx_planar_map_download(vgx_planar_map M, uint8_t* state, int8_t* occupancy, float* clearance, float* height, float* distance) {
  if (!M) return VGX_ERR_INVALID;
  vgx_ctx ctx = M->ctx;
  std::lock_guard<std::mutex> lk(M->mu);
  const size_t n = (size_t)M->W * (size_t)M->H;
  if (n == 0) return VGX_OK;
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the map was complete when its producer returned, whichever stream made it)
  if (state) VGX_HIP(ctx, hipMemcpyAsync(state, M->d_state.p, n, hipMemcpyDeviceToHost, st));
  if (occupancy) VGX_HIP(ctx, hipMemcpyAsync(occupancy, M->d_occupancy.p, n, hipMemcpyDeviceToHost, st));
  if (clearance) VGX_HIP(ctx, hipMemcpyAsync(clearance, M->d_clearance.p, n * 4, hipMemcpyDeviceToHost, st));
  if (height) VGX_HIP(ctx, hipMemcpyAsync(height, M->d_height.p, n * 4, hipMemcpyDeviceToHost, st));
  if (distance) VGX_HIP(ctx, hipMemcpyAsync(distance, M->d_distance.p, n * 4, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  return VGX_OK;
}

int vgx_submap_layer_planar_map(vgx_submap sm, int32_t layer, const vgx_planar_map_config* cfg, vgx_planar_map M) {
  static const char* kFn = "vgx_submap_layer_planar_map";
  if (!sm) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL submap");
  vgx_ctx ctx = sm->ctx;
  PlanarRule rule{};
  int rc = planar_check(ctx, kFn, cfg, M, sm->voxel_size, &rule);
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
  return planar_generate(ctx, kFn, ctx->stream, tsdf ? kCloudSrcTsdf : kCloudSrcEsdf, sm->vps, s, t, rule, *cfg, sm->n_blocks, M);
}

int vgx_tsdf_layer_planar_map(vgx_tsdf_layer L, const vgx_planar_map_config* cfg, vgx_planar_map M) {
  static const char* kFn = "vgx_tsdf_layer_planar_map";
  if (!L) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL layer");
  vgx_ctx ctx = L->ctx;
  PlanarRule rule{};
  int rc = planar_check(ctx, kFn, cfg, M, L->dev.voxel_size, &rule);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> map_lk(M->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  CloudSrc s{};
  PlanarTable t{};
  rc = planar_layer_source(L, kFn, &s, &t);
  if (rc != VGX_OK) return rc;
  const TsdfLayerDev& d = L->dev;
  return planar_generate(ctx, kFn, ctx->tsdf_stream, kCloudSrcPacked, d.vps, s, t, rule, *cfg, d.max_blocks, M);
}

}  // extern "C"
