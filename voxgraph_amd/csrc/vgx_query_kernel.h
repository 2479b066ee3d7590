// The map-query kernel (vgx_submap_query / _device, include/voxgraph_amd.h): voxblox's EsdfMap / TsdfMap lookups
// [recalled] at arbitrary points of a finished submap's raw ESDF or TSDF layer.  One thread per query.  The rules are
// stated in the header; the layout read and the window route in DESIGN.md 14.  The interpolated gradient has two routes, the
// window route and the generic one (vgx_query.hip picks; a profiling build forces the generic one).  Only the indices
// decide which voxels are read, so both routes give the same bits.
#ifndef VGX_QUERY_KERNEL_H_
#define VGX_QUERY_KERNEL_H_

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>

#include "vgx_internal.h"
#include "vgx_interp.h"
#include "vgx_pose.h"

#pragma clang fp contract(off)

namespace vgx {

struct QueryDev : LayerTable {  // (the submap's raw layer)
  const float* val;  // ESDF or TSDF distance
  const void* vld;   // ESDF observed (uint8) or TSDF weight (float)
  int32_t posed;
  int32_t offsets32;       // n_blocks * vps^3 < 2^32: the window route's loads take 32-bit offsets
  float q_qs[4];           // T_Q_S rotation {w, x, y, z}: gradients back into the query frame
  float q_sq[4], t_sq[3];  // T_S_Q = T_Q_S.inverse(): query points into the submap frame
  const float* points;     // [n][3]
  float* distance;         // [n]
  float* gradient;         // [n][3] (GRAD instances only)
  float* weight;           // [n] or null (TSDF only)
  uint8_t* valid;          // [n]
  int64_t n;
};

constexpr int kQueryThreads = 256;

// Interpolator::getNearestDistance [recalled]: p's own voxel (vgx_interp.h's floor rule, clamped into the block), which
// must exist and be valid; its own distance and (TSDF) weight
template <int VPS, bool TSDF>
__device__ __forceinline__ bool query_nearest(const QueryDev& q, const float pos[3], float& d, float& w) {
  int b[3], v[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    b[a] = (int)floorf(pos[a] * q.block_size_inv + 1e-6f);
    const float origin = (float)b[a] * q.block_size;
    v[a] = min(max((int)floorf((pos[a] - origin) * q.voxel_size_inv + 1e-6f), 0), VPS - 1);
  }
  const int slot = interp_slot(q, b[0], b[1], b[2]);
  if (slot < 0) return false;
  const size_t at = (size_t)slot * (VPS * VPS * VPS) + (size_t)(v[0] + VPS * (v[1] + VPS * v[2]));
  d = q.val[at];
  if (TSDF) {
    w = static_cast<const float*>(q.vld)[at];
    return interp_valid(w);
  }
  return interp_valid(static_cast<const uint8_t*>(q.vld)[at]);
}

// Interpolator::getDistance(p, &d, interpolate) [recalled]
template <int VPS, bool TSDF, bool INTERP>
__device__ __forceinline__ bool query_distance(const QueryDev& q, const float pos[3], float& d, float& w) {
  if (!INTERP) return query_nearest<VPS, TSDF>(q, pos, d, w);
  if (TSDF) return layer_interp<VPS>(q, q.val, static_cast<const float*>(q.vld), pos, d, w);
  return layer_interp<VPS>(q, q.val, static_cast<const uint8_t*>(q.vld), pos, d, w);
}

// The window route.  The 7 interpolations of an interpolated gradient (the centre, then x-, x+, y-, y+, z-, z+) almost
// always have the low neighbours G0, G0 - e_a and G0 + e_a (global voxel indices): their cubes are then sub-cubes of the
// 4x4x4 window from G0 - 1, and together read only its 32 cells {1,2}^3 (ids 0..7) and, per axis a and side s, the 4
// cells with c_a = 0 / 3 and the other two coordinates in {1,2} (ids 8 + 4 (2a + s) ..).
__host__ __device__ constexpr int win_id(int x, int y, int z) {
  return (x >= 1 && x <= 2 && y >= 1 && y <= 2 && z >= 1 && z <= 2) ? (x - 1) * 4 + (y - 1) * 2 + (z - 1)
         : (x == 0 || x == 3) ? 8 + 4 * (x == 3 ? 1 : 0) + (y - 1) * 2 + (z - 1)
         : (y == 0 || y == 3) ? 16 + 4 * (y == 3 ? 1 : 0) + (x - 1) * 2 + (z - 1)
                              : 24 + 4 * (z == 3 ? 1 : 0) + (x - 1) * 2 + (y - 1);
}
// the inverse of win_id: coordinate a of cell id
__host__ __device__ constexpr int win_coord(int id, int a) {
  return id < 8 ? 1 + ((id >> (2 - a)) & 1)
         : a == ((id - 8) >> 3) ? ((((id - 8) >> 2) & 1) ? 3 : 0)
         : a == (((id - 8) >> 3) == 0 ? 1 : 0) ? 1 + ((id >> 1) & 1)
                                               : 1 + (id & 1);
}
static_assert(win_id(win_coord(13, 0), win_coord(13, 1), win_coord(13, 2)) == 13, "win_coord inverts win_id");
static_assert(win_id(1, 1, 1) == 0 && win_id(1, 1, 2) == 1 && win_id(2, 2, 2) == 7, "the centre cube is ids 0..7 in neighbour order");


// one window cell, its id a constant: the block among the 8 candidates (lo + bits), then its distance and validity (and,
// for the centre cube's cells, its TSDF weight)
template <int VPS, bool TSDF, int ID>
__device__ __forceinline__ void win_load(const QueryDev& q, const int (&cv)[3][4], const int (&cb)[3][4], const int (&slot)[8],
                                         float (&cd)[32], float (&cw)[8], bool& all) {
  constexpr int VOX = VPS * VPS * VPS;
  constexpr int cx = win_coord(ID, 0), cy = win_coord(ID, 1), cz = win_coord(ID, 2);
  const int h = cb[0][cx] | (cb[1][cy] << 1) | (cb[2][cz] << 2);
  int s = slot[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) s = h == j ? slot[j] : s;
  cd[ID] = 0.0f;
  if (ID < 8) cw[ID & 7] = 0.0f;
  if (s < 0) {
    all = false;
    return;
  }
  // 32-bit voxel offsets (q.offsets32: the layer has < 2^32 voxels) let every load use the layer's base in SGPRs
  const uint32_t at = (uint32_t)s * VOX + (uint32_t)(cv[0][cx] + VPS * (cv[1][cy] + VPS * cv[2][cz]));
  cd[ID] = q.val[at];
  if (TSDF) {
    const float wv = static_cast<const float*>(q.vld)[at];
    if (ID < 8) cw[ID & 7] = wv;
    all = all && interp_valid(wv);
  } else {
    all = all && interp_valid(static_cast<const uint8_t*>(q.vld)[at]);
  }
}
template <int VPS, bool TSDF, int BASE, int... IDs>
__device__ __forceinline__ void win_load_all(std::integer_sequence<int, IDs...>, const QueryDev& q, const int (&cv)[3][4],
                                             const int (&cb)[3][4], const int (&slot)[8], float (&cd)[32], float (&cw)[8],
                                             bool& all) {
  (win_load<VPS, TSDF, BASE + IDs>(q, cv, cb, slot, cd, cw, all), ...);
}

// interpolation K of the 7 (the centre, then x-, x+, y-, y+, z-, z+) from the window's cells: its cube's low corner is
// (1,1,1) + s e_a
template <int K>
__device__ __forceinline__ void win_interp(const float (&cd)[32], const float (&dl)[7][3], float (&dk)[7]) {
  constexpr int a = K == 0 ? 0 : (K - 1) >> 1;
  constexpr int s = K == 0 ? 0 : (((K - 1) & 1) ? 1 : -1);
  constexpr int b0 = 1 + (a == 0 ? s : 0), b1 = 1 + (a == 1 ? s : 0), b2 = 1 + (a == 2 ? s : 0);
  const float x[8] = {cd[win_id(b0, b1, b2)],         cd[win_id(b0, b1, b2 + 1)],         cd[win_id(b0, b1 + 1, b2)],
                      cd[win_id(b0, b1 + 1, b2 + 1)], cd[win_id(b0 + 1, b1, b2)],         cd[win_id(b0 + 1, b1, b2 + 1)],
                      cd[win_id(b0 + 1, b1 + 1, b2)], cd[win_id(b0 + 1, b1 + 1, b2 + 1)]};
  dk[K] = interp_trilinear(x, dl[K]);
}
template <int... Ks>
__device__ __forceinline__ void win_interp_all(std::integer_sequence<int, Ks...>, const float (&cd)[32], const float (&dl)[7][3],
                                               float (&dk)[7]) {
  (win_interp<Ks>(cd, dl, dk), ...);
}

template <int VPS, bool TSDF, bool INTERP, bool GRAD, bool WINDOW>
__global__ __launch_bounds__(kQueryThreads) __attribute__((amdgpu_waves_per_eu(4))) void query_kernel(QueryDev q) {
  const int64_t i = (int64_t)blockIdx.x * kQueryThreads + threadIdx.x;
  if (i >= q.n) return;
  float x[3] = {q.points[3 * i], q.points[3 * i + 1], q.points[3 * i + 2]};
  float p[3];
  if (q.posed) {
    quat_rotate(q.q_sq, x, p);  // (rigid_apply's two steps written out: through the helper the gradient instantiations spilled)
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = p[a] + q.t_sq[a];
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = x[a];
  }
  // a coordinate whose block index would leave [-2^30, 2^30) -- every non-finite one -- makes the query invalid.  (The
  // rule stays written out in each reader: as a shared predicate it took the gradient instantiations here from 95 / 108
  // VGPRs to 128 with 12 to 52 bytes of scratch, the localisation kernel into the next VGPR granule, and the view
  // kernel's LiDAR case 5 % of its time.)
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && fabsf(p[a] * q.block_size_inv) < 1073741824.0f;
  float d = 0.0f, w = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
  if (ok) {
    if (!GRAD) {
      ok = query_distance<VPS, TSDF, INTERP>(q, p, d, w);
    } else {
      // the centre (k = 0) and p +- voxel_size e_a (k = 1 + 2a + (s > 0))
      float pk[7][3];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) pk[k][a] = p[a];
        if (k > 0) {
          const int a = (k - 1) >> 1;
          pk[k][a] = ((k - 1) & 1) ? p[a] + q.voxel_size : p[a] - q.voxel_size;
        }
      }
      float dk[7];
      bool window = false;
      if (INTERP && WINDOW) {
        int blk[7][3], vox[7][3];
        float dl[7][3];
#pragma unroll
        for (int k = 0; k < 7; ++k) interp_base<VPS>(q, pk[k], blk[k], vox[k], dl[k]);
        window = true;
#pragma unroll
        for (int k = 1; k < 7; ++k) {
          const int a = (k - 1) >> 1, s = ((k - 1) & 1) ? 1 : -1;
#pragma unroll
          for (int b = 0; b < 3; ++b)
            window = window && (blk[k][b] - blk[0][b]) * VPS + (vox[k][b] - vox[0][b]) == (b == a ? s : 0);
        }
        window = window && q.offsets32;
        if (window) {
          // per axis: cell c of the window is voxel vox0 - 1 + c of block blk0 + off, off in {-1, 0, 1}; the window spans
          // two blocks at most per axis (VPS >= 8): lo = blk0 - (vox0 == 0), the cell's bit says lo or lo + 1
          int cv[3][4], cb[3][4], lo[3];
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            lo[a] = blk[0][a] - (vox[0][a] == 0 ? 1 : 0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int u = vox[0][a] - 1 + c;
              const int off = u < 0 ? -1 : (u >= VPS ? 1 : 0);
              cv[a][c] = u - off * VPS;
              cb[a][c] = blk[0][a] + off - lo[a];
            }
          }
          int slot[8];
#pragma unroll
          for (int h = 0; h < 8; ++h) slot[h] = interp_slot(q, lo[0] + (h & 1), lo[1] + ((h >> 1) & 1), lo[2] + (h >> 2));
          float cd[32], cw[8];
          bool all = true;
          // the centre cube first: a query whose distance fails is invalid whatever its gradient (most of the points far
          // from an observed surface), so the 24 face cells are read only after it held
          win_load_all<VPS, TSDF, 0>(std::make_integer_sequence<int, 8>{}, q, cv, cb, slot, cd, cw, all);
          if (all) win_load_all<VPS, TSDF, 8>(std::make_integer_sequence<int, 24>{}, q, cv, cb, slot, cd, cw, all);
          ok = all;
          if (ok) win_interp_all(std::make_integer_sequence<int, 7>{}, cd, dl, dk);
          if (ok && TSDF) {
            float xw[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) xw[n] = cw[n];  // (the centre cube's cells are ids 0..7 in neighbour order)
            w = interp_trilinear(xw, dl[0]);
          }
        }
      }
      if (!window) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          float wk = 0.0f;
          ok = ok && query_distance<VPS, TSDF, INTERP>(q, pk[k], dk[k], wk);
          if (k == 0) w = wk;
        }
      }
      if (ok) {
        d = dk[0];
        const float two_vs = 2.0f * q.voxel_size;
        float gs[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) gs[a] = (dk[2 + 2 * a] - dk[1 + 2 * a]) / two_vs;
        if (q.posed) {
          quat_rotate(q.q_qs, gs, g);
        } else {
#pragma unroll
          for (int a = 0; a < 3; ++a) g[a] = gs[a];
        }
      }
    }
  }
  if (!ok) {
    d = 0.0f;
    w = 0.0f;
    g[0] = g[1] = g[2] = 0.0f;
  }
  q.distance[i] = d;
  q.valid[i] = ok ? 1 : 0;
  if (GRAD) {
    q.gradient[3 * i] = g[0];
    q.gradient[3 * i + 1] = g[1];
    q.gradient[3 * i + 2] = g[2];
  }
  if (TSDF && q.weight) q.weight[i] = w;
}

// one launch: the instance for (vps, layer, interpolate, gradient); `window` false forces the generic route
template <bool WINDOW>
inline hipError_t launch_query(hipStream_t st, const QueryDev& q, int vps, bool tsdf, bool interp, bool grad) {
  const int64_t blocks = (q.n + kQueryThreads - 1) / kQueryThreads;
  void (*k)(QueryDev) = nullptr;
#define VGX_QUERY_PICK(V)                                                                                           \
  k = tsdf ? (interp ? (grad ? query_kernel<V, true, true, true, WINDOW> : query_kernel<V, true, true, false, WINDOW>)   \
                     : (grad ? query_kernel<V, true, false, true, WINDOW> : query_kernel<V, true, false, false, WINDOW>)) \
           : (interp ? (grad ? query_kernel<V, false, true, true, WINDOW> : query_kernel<V, false, true, false, WINDOW>) \
                     : (grad ? query_kernel<V, false, false, true, WINDOW> : query_kernel<V, false, false, false, WINDOW>))
  if (vps == 16) {
    VGX_QUERY_PICK(16);
  } else {
    VGX_QUERY_PICK(8);
  }
#undef VGX_QUERY_PICK
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kQueryThreads), 0, st, q);
  return hipGetLastError();
}

inline int query_fail(vgx_ctx ctx, const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, "vgx_submap_query: " + msg); }

// The checks of both calls (refused before anything is written), then the kernel's descriptor.  Returns VGX_OK with
// *run = false when there is nothing to do (n = 0).
inline int query_prepare(vgx_submap sm, int32_t layer, int32_t flags, const float* T_Q_S, int64_t n, const void* points,
                  const void* distance, const void* gradient, const void* weight, const void* valid, QueryDev& q, bool& run) {
  run = false;
  if (!sm) return VGX_ERR_INVALID;
  vgx_ctx ctx = sm->ctx;
  if (n < 0) return query_fail(ctx, "n < 0");
  if (n > 0 && (!points || !distance || !valid)) return query_fail(ctx, "NULL points / distance / valid with n > 0");
  if (flags & ~(VGX_QUERY_INTERPOLATE | VGX_QUERY_GRADIENT)) return query_fail(ctx, "unknown flag bits");
  if (layer != VGX_EVAL_LAYER_ESDF && layer != VGX_EVAL_LAYER_TSDF) return query_fail(ctx, "layer is neither ESDF nor TSDF");
  if ((flags & VGX_QUERY_GRADIENT) && !gradient) return query_fail(ctx, "VGX_QUERY_GRADIENT without a gradient array");
  if (weight && layer == VGX_EVAL_LAYER_ESDF) return query_fail(ctx, "a weight array on an ESDF query");
  const bool tsdf = layer == VGX_EVAL_LAYER_TSDF;
  if (sm->n_blocks > 0 && (tsdf ? !(sm->d_tsdf_distance && sm->d_tsdf_weight) : !(sm->d_esdf_distance && sm->d_esdf_observed)))
    return query_fail(ctx, std::string(tsdf ? "TSDF" : "ESDF") + " layer not resident (released, or never generated)");
  if (T_Q_S) {
    const PoseDefect bad = pose_defect(T_Q_S);
    if (bad == kPoseNotFinite) return query_fail(ctx, "pose value not finite");
    if (bad == kPoseNotUnit) return query_fail(ctx, "pose quaternion not unit (|q|^2 - 1 > 1e-4)");
  }
  if (sm->vps != 8 && sm->vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_submap_query: voxels_per_side not 8 or 16");
  if ((n + kQueryThreads - 1) / kQueryThreads > 0x7fffffffll) return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_submap_query: n too large for one launch");
  if (n == 0) return VGX_OK;
  q = QueryDev{};
  static_cast<LayerTable&>(q) = submap_table(sm);
  q.val = tsdf ? sm->d_tsdf_distance : sm->d_esdf_distance;
  q.vld = tsdf ? (const void*)sm->d_tsdf_weight : (const void*)sm->d_esdf_observed;
  q.posed = T_Q_S ? 1 : 0;
  q.offsets32 = (uint64_t)sm->n_blocks * (uint64_t)(sm->vps * sm->vps * sm->vps) < (1ull << 32) ? 1 : 0;
  if (T_Q_S) {
    for (int k = 0; k < 4; ++k) q.q_qs[k] = T_Q_S[k];
    inverse_pose(T_Q_S, T_Q_S + 4, q.q_sq, q.t_sq);  // T_S_Q, once in f32
  }
  q.n = n;
  run = true;
  return VGX_OK;
}

}  // namespace vgx

#endif  // VGX_QUERY_KERNEL_H_
