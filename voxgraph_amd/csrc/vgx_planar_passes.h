// The passes the 2D map products share: the planar map (vgx_planar.hip) and the elevation map (vgx_elevation.hip).
//   planar_band_rows      which rows of a z block lie in the height band (host and device: one comparison for both)
//   planar_box_kernel     the x/y extent of the blocks with a row in the band
//   planar_row_kernel     g[y][x] = the distance in cells to the nearest obstacle cell of row y within R, or none (u16)
//   planar_column_kernel  d2 = min over |dy| <= R of dy^2 + g[y + dy][x]^2 (int); then sqrtf, the voxel size and the clip
// The row pass takes the obstacle predicate as a functor over the product's per-cell byte (the planar map's state, the
// elevation map's class).  The rules are stated in include/voxgraph_amd.h, "Planar map", `box` and `distance`.
#ifndef VGX_PLANAR_PASSES_H_
#define VGX_PLANAR_PASSES_H_

#include <climits>
#include <cmath>
#include <string>

#include "vgx_cloud_src.h"
#include "vgx_internal.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

constexpr int kPlanarTile = 16;         // gather: cells per workgroup side
constexpr int kPlanarPassX = 32;        // row and column passes: a workgroup is 32 x 8 cells
constexpr int kPlanarPassY = 8;
constexpr uint16_t kPlanarNone = 0xffffu;
constexpr int kPlanarMaxR = 2048;
constexpr int32_t kPlanarBoxInit = 0x7f7f7f7f;  // what a memset of 0x7f leaves: above every block index (|index| < 2^28)
constexpr long long kPlanarMaxCells = 1ll << 28;

// the layer's dense block table: [dim.z][dim.y][dim.x] -> slot of the block pool, or < 0
struct PlanarTable {
  const int32_t* lut;
  int32_t lut_min[3], lut_dim[3];
  int32_t slots;  // of the block pool: an entry at or beyond it is never followed
};

struct PlanarBox {
  int32_t x0, y0, W, H;
  long long tx0, ty0;  // x0, y0 rounded down to the gather tile
  int32_t tiles_x, tiles_y;
};

// Bit i: row i (on z) of a block with z index bz is in the band, z_min <= cz && cz <= z_max.  From the block index
// alone: 0 rejects the block before any voxel is read, and the rows of a kept block test their bit -- the same
// comparison either way.  Host and device (the host finds [bz_lo, bz_hi] with it).
template <int VPS>
__host__ __device__ __forceinline__ uint32_t planar_band_rows(float z_min, float z_max, int bz, float vs) {
  const float origin = (float)bz * ((float)VPS * vs);
  uint32_t rows = 0;
#pragma unroll
  for (int i = 0; i < VPS; ++i) {
    const float cz = voxel_centre(origin, i, vs);
    if (z_min <= cz && cz <= z_max) rows |= 1u << i;
  }
  return rows;
}

// the obstacle cells of both products: the byte is 2, or 0 where unknown cells count as obstacles
struct PlanarObstacle {
  int unknown_is_obstacle;
  __device__ __forceinline__ bool operator()(uint8_t v) const { return v == 2 || (unknown_is_obstacle != 0 && v == 0); }
};

// box[4] = min of {bx, by, -bx, -by} over the live blocks with a row in the band (kPlanarBoxInit where there is none)
template <int VPS>
__global__ __launch_bounds__(256) void planar_box_kernel(CloudSrc s, float z_min, float z_max, int slots, int32_t* __restrict__ box) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  int v[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
  if (b < (long long)cloud_live_blocks(s, slots)) {
    const int32_t* bi = s.block_index + 3 * (size_t)b;
    if (planar_band_rows<VPS>(z_min, z_max, bi[2], s.voxel_size) != 0u) {
      v[0] = bi[0];
      v[1] = bi[1];
      v[2] = -bi[0];
      v[3] = -bi[1];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] = min(v[k], __shfl_xor(v[k], o));
  }
  if ((threadIdx.x & 63) == 0 && v[0] != INT_MAX) {
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicMin(box + k, v[k]);
  }
}

template <class Obstacle>
__global__ __launch_bounds__(256) void planar_row_kernel(const uint8_t* __restrict__ cells, int W, int H, int tiles_x, int R,
                                                         Obstacle obstacle, uint16_t* __restrict__ g) {
  const int x = kPlanarPassX * (int)(blockIdx.x % (unsigned)tiles_x) + (int)(threadIdx.x % kPlanarPassX);
  const int y = kPlanarPassY * (int)(blockIdx.x / (unsigned)tiles_x) + (int)(threadIdx.x / kPlanarPassX);
  if (x >= W || y >= H) return;
  const uint8_t* row = cells + (size_t)y * (size_t)W;
  int best = kPlanarNone;
  if (obstacle(row[x])) {
    best = 0;
  } else {
    for (int k = 1; k <= R; ++k) {
      const bool left = x - k >= 0, right = x + k < W;
      if (!left && !right) break;
      if ((left && obstacle(row[x - k])) || (right && obstacle(row[x + k]))) {
        best = k;
        break;
      }
    }
  }
  g[(size_t)y * (size_t)W + (size_t)x] = (uint16_t)best;
}

static __global__ __launch_bounds__(256) void planar_column_kernel(const uint16_t* __restrict__ g, int W, int H, int tiles_x, int R,
                                                                   float voxel_size, float max_distance_m,
                                                                   float* __restrict__ distance) {
  const int x = kPlanarPassX * (int)(blockIdx.x % (unsigned)tiles_x) + (int)(threadIdx.x % kPlanarPassX);
  const int y = kPlanarPassY * (int)(blockIdx.x / (unsigned)tiles_x) + (int)(threadIdx.x / kPlanarPassX);
  if (x >= W || y >= H) return;
  const uint16_t* col = g + (size_t)x;
  int best = INT_MAX;  // none
  const int g0 = col[(size_t)y * (size_t)W];
  if (g0 != kPlanarNone) best = g0 * g0;
  for (int dy = 1; dy <= R; ++dy) {
    const int dy2 = dy * dy;
    if (dy2 >= best) break;  // no later row can be nearer
    const bool up = y - dy >= 0, down = y + dy < H;
    if (!up && !down) break;
    if (up) {
      const int gg = col[(size_t)(y - dy) * (size_t)W];
      if (gg != kPlanarNone) best = min(best, dy2 + gg * gg);
    }
    if (down) {
      const int gg = col[(size_t)(y + dy) * (size_t)W];
      if (gg != kPlanarNone) best = min(best, dy2 + gg * gg);
    }
  }
  float out = max_distance_m;
  if (best != INT_MAX) {
    const float m = sqrtf((float)best) * voxel_size;
    out = m < max_distance_m ? m : max_distance_m;
  }
  distance[(size_t)y * (size_t)W + (size_t)x] = out;
}

// Host side, shared by the two products' producers -----------------------------------------------------------------

// ix = block_x * vps + local_x must fit int32 for every block the table can hold, on x and y
inline bool planar_table_fits(const int32_t lut_min[3], const int32_t lut_dim[3], int vps) {
  for (int a = 0; a < 2; ++a) {
    if (lut_dim[a] <= 0) continue;
    const long long lo = (long long)lut_min[a] * vps, hi = ((long long)lut_min[a] + lut_dim[a]) * vps - 1;
    if (lo < (long long)INT32_MIN || hi > (long long)INT32_MAX) return false;
  }
  return true;
}

inline long long planar_floor_to(long long v, long long m) { return v >= 0 ? v / m * m : -((-v + m - 1) / m) * m; }

// the table's z blocks with a row in the band, [*bz_lo, *bz_hi] (left as they were where there is none): the very
// comparison of the kernels
inline void planar_band_blocks(const PlanarTable& t, int vps, float z_min, float z_max, float voxel_size, int32_t* bz_lo, int32_t* bz_hi) {
  if (t.lut_dim[0] <= 0 || t.lut_dim[1] <= 0) return;
  for (int k = 0; k < t.lut_dim[2]; ++k) {
    const int bz = t.lut_min[2] + k;
    const uint32_t rows = vps == 16 ? planar_band_rows<16>(z_min, z_max, bz, voxel_size) : planar_band_rows<8>(z_min, z_max, bz, voxel_size);
    if (rows == 0u) continue;
    if (*bz_lo > *bz_hi) *bz_lo = bz;
    *bz_hi = bz;
  }
}

inline PlanarBox planar_make_box(long long x0, long long y0, long long W, long long H) {
  PlanarBox b{};
  b.x0 = (int32_t)x0;
  b.y0 = (int32_t)y0;
  b.W = (int32_t)W;
  b.H = (int32_t)H;
  b.tx0 = planar_floor_to(x0, kPlanarTile);
  b.ty0 = planar_floor_to(y0, kPlanarTile);
  b.tiles_x = (int32_t)((x0 + W - b.tx0 + kPlanarTile - 1) / kPlanarTile);
  b.tiles_y = (int32_t)((y0 + H - b.ty0 + kPlanarTile - 1) / kPlanarTile);
  return b;
}

// The grid box of a producing call, box = {x0, y0, W, H}: the given one, or the extent of the band's blocks from the box
// kernel and the first host synchronisation (`band`: the table has a z block with a row in the band).  ev: two events to
// record either side of the box kernel, or null; *ran: the kernel ran between them.
inline int planar_find_box(vgx_ctx ctx, const char* fn, hipStream_t st, int vps, const CloudSrc& s, float z_min, float z_max, bool band,
                           int slots, int32_t use_box, const int32_t cell_min[2], const int32_t cell_dim[2], int32_t* d_box, hipEvent_t* ev,
                           long long box[4], bool* ran) {
  box[0] = box[1] = box[2] = box[3] = 0;
  *ran = false;
  if (use_box != 0) {
    box[0] = cell_min[0];
    box[1] = cell_min[1];
    box[2] = cell_dim[0];
    box[3] = cell_dim[1];
  } else if (slots > 0 && band) {
    int32_t got[4];
    VGX_HIP(ctx, hipMemsetAsync(d_box, 0x7f, 16, st));
    const unsigned groups = (unsigned)(((long long)slots + 255) / 256);
    if (ev) VGX_HIP(ctx, hipEventRecord(ev[0], st));
    if (vps == 16) hipLaunchKernelGGL(planar_box_kernel<16>, dim3(groups), dim3(256), 0, st, s, z_min, z_max, slots, d_box);
    else hipLaunchKernelGGL(planar_box_kernel<8>, dim3(groups), dim3(256), 0, st, s, z_min, z_max, slots, d_box);
    VGX_HIP(ctx, hipGetLastError());
    if (ev) VGX_HIP(ctx, hipEventRecord(ev[1], st));
    *ran = true;
    VGX_HIP(ctx, hipMemcpyAsync(got, d_box, 16, hipMemcpyDeviceToHost, st));
    VGX_HIP(ctx, hipStreamSynchronize(st));
    if (got[0] != kPlanarBoxInit) {
      box[0] = (long long)got[0] * vps;
      box[1] = (long long)got[1] * vps;
      box[2] = ((long long)-got[2] - got[0] + 1) * vps;
      box[3] = ((long long)-got[3] - got[1] + 1) * vps;
    }
    if (box[2] * box[3] > kPlanarMaxCells)
      return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": the band's blocks span more than 2^28 cells");
  }
  return VGX_OK;
}

// A finished submap's raw TSDF or ESDF layer as a source; the caller holds the registration lock, under which the
// submap's layers and block table are read (another thread may release or generate them).
inline int planar_submap_source(vgx_submap sm, bool tsdf, const char* fn, CloudSrc* s, PlanarTable* t) {
  vgx_ctx ctx = sm->ctx;
  if (sm->n_blocks > 0 && (tsdf ? (!sm->d_tsdf_distance || !sm->d_tsdf_weight) : (!sm->d_esdf_distance || !sm->d_esdf_observed)))
    return set_error(ctx, VGX_ERR_INVALID,
                     std::string(fn) + (tsdf ? ": TSDF" : ": ESDF") + " layer not resident (released, or never generated)");
  if (sm->vps != 8 && sm->vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": voxels_per_side must be 8 or 16");
  if (!planar_table_fits(sm->lut_min, sm->lut_dim, sm->vps))
    return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": block indices overflow the int32 voxel index");
  *s = CloudSrc{};
  s->block_index = sm->d_block_index;
  s->dist = tsdf ? sm->d_tsdf_distance : sm->d_esdf_distance;
  s->seen = tsdf ? (const void*)sm->d_tsdf_weight : (const void*)sm->d_esdf_observed;
  s->voxel_size = sm->voxel_size;
  *t = PlanarTable{};
  t->lut = sm->d_lut;
  for (int a = 0; a < 3; ++a) {
    t->lut_min[a] = sm->lut_min[a];
    t->lut_dim[a] = sm->n_blocks > 0 ? sm->lut_dim[a] : 0;
  }
  t->slots = sm->n_blocks;
  return VGX_OK;
}

// A vgx_tsdf_layer as a source; the caller holds the TSDF lock.
inline int planar_layer_source(vgx_tsdf_layer L, const char* fn, CloudSrc* s, PlanarTable* t) {
  vgx_ctx ctx = L->ctx;
  const TsdfLayerDev& d = L->dev;
  if (d.vps != 8 && d.vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": voxels_per_side must be 8 or 16");
  if (!planar_table_fits(d.lut_min, d.lut_dim, d.vps))
    return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": block indices overflow the int32 voxel index");
  *s = CloudSrc{};
  s->block_index = d.block_index;
  // behind the scans and merges queued on the TSDF stream, whose allocation counter only the device knows
  s->live_blocks = d.n_blocks;
  s->live_blocks_is_64 = 0;
  s->words = d.voxels;
  s->rgba = d.rgba;
  s->voxel_size = d.voxel_size;
  *t = PlanarTable{};
  t->lut = d.lut;
  for (int a = 0; a < 3; ++a) {
    t->lut_min[a] = d.lut_min[a];
    t->lut_dim[a] = d.lut ? d.lut_dim[a] : 0;
  }
  t->slots = d.max_blocks;
  return VGX_OK;
}

}  // namespace vgx

#endif
