// Scan localisation (include/voxgraph_amd.h, "Scan localisation"): a scan's points against the ESDF or
// TSDF of posed, finished submaps -- one evaluation at a pose, many poses scored in one call, the best one refined.  The
// formulation and the order contract are stated in the header; tests/scan_localization_ref.py restates every bit.
//
//   1. scan_map_eval_kernel<VPS, TSDF, FULL>: "Scan-to-map registration"'s partition (candidate j to slot j / 1024,
//      thread (j % 1024) % 256, trip (j % 1024) / 256).  Per candidate one rotation into the mission frame; per submap,
//      in ascending order, one rigid transform, the block-table lookups of the 8 neighbours, then their 8 + 8 gathers
//      (distance and validity are two raw arrays), the residual and -- FULL -- the exact gradient rotated back.  FULL
//      keeps 15 f64 sums and three counts; the cost-only instantiation one sum and three counts, no gradient, and serves
//      workgroup b's pose b / groups and slot b % groups, reading the pose from a table.
//   2. scan_map_fold_kernel<NS>: one workgroup of 256 threads per pose folds that pose's partials in slot order.
// One D2H copy into the handle's pinned stage and one synchronisation per call.  No float atomics.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "vgx_internal.h"
#include "vgx_interp.h"
#include "vgx_query_kernel.h"
#include "vgx_scan_reg_internal.h"

#pragma clang fp contract(off)

namespace vgx {

constexpr int kScanMapCounts = 3;  // n_terms, n_points_valid, n_candidates

template <int NS>
struct ScanMapSums {  // FULL: 144 B; cost-only: 32 B
  double s[NS];
  long long n[kScanMapCounts];
};

struct ScanMapDev {
  const ScanMapSubmapDev* submaps;  // [n_submaps]
  int32_t n_submaps;
  int32_t stride;
  const float* points;              // [n][3] sensor frame
  long long n_strided;              // candidates by stride alone: ceil(n / stride)
  const float* poses;               // cost-only: [n_poses][7], {q, t'}
  int32_t groups;                   // cost-only: slots per pose
  float q[4], t[3];                 // FULL: the prior's rotation; t' = (float)((double)t_prior + delta)
  float c, s;                       // FULL: (float)cos / sin(delta yaw)
  float min_range2, max_range2, max_abs_distance;
  double huber;                     // (double)huber_delta_m
  void* partials;                   // ScanMapSums<NS> [workgroups]
};

// "Scan-to-map registration"'s tree over any number of sums: the 64 lanes by v[l] += v[l + o], o = 32 .. 1; lane 0 of
// every wave then holds its wave's sums: the waves in order, by thread 0 -> out
template <int WAVES, int NS>
__device__ __forceinline__ void scan_map_block_fold(ScanMapSums<NS>& v, ScanMapSums<NS>* out) {
  __shared__ double sh[WAVES][NS];
  __shared__ long long sh_n[WAVES][kScanMapCounts];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < NS; ++k) v.s[k] += __shfl_down(v.s[k], o);
#pragma unroll
    for (int k = 0; k < kScanMapCounts; ++k) v.n[k] += __shfl_down(v.n[k], o);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) sh[w][k] = v.s[k];
#pragma unroll
    for (int k = 0; k < kScanMapCounts; ++k) sh_n[w][k] = v.n[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScanMapSums<NS> p;
#pragma unroll
    for (int k = 0; k < NS; ++k) p.s[k] = sh[0][k];
#pragma unroll
    for (int k = 0; k < kScanMapCounts; ++k) p.n[k] = sh_n[0][k];
    for (int i = 1; i < WAVES; ++i) {  // the waves in order
#pragma unroll
      for (int k = 0; k < NS; ++k) p.s[k] += sh[i][k];
#pragma unroll
      for (int k = 0; k < kScanMapCounts; ++k) p.n[k] += sh_n[i][k];
    }
    *out = p;
  }
}

template <int VPS, bool TSDF, bool FULL>
__global__ __launch_bounds__(kScanRegThreads) void scan_map_eval_kernel(ScanMapDev d) {
  constexpr int VOX = VPS * VPS * VPS;
  constexpr int NS = FULL ? kScanRegSums : 1;
  ScanMapSums<NS> acc;
#pragma unroll
  for (int k = 0; k < NS; ++k) acc.s[k] = 0.0;
  long long n_terms = 0, n_valid = 0, n_cand = 0;
  // the pose: FULL the prior and the correction of the descriptor; cost-only row (workgroup / groups) of the table at
  // delta = 0, i.e. c = 1, s = 0 in the same expressions (the compiler folds what IEEE lets it fold)
  float pq[4], pt[3];
  long long slot = blockIdx.x;
  if (FULL) {
#pragma unroll
    for (int k = 0; k < 4; ++k) pq[k] = d.q[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) pt[a] = d.t[a];
  } else {
    const unsigned pose = blockIdx.x / (unsigned)d.groups;
    slot = blockIdx.x - pose * (unsigned)d.groups;
    const float* __restrict__ T = d.poses + 7 * (size_t)pose;
#pragma unroll
    for (int k = 0; k < 4; ++k) pq[k] = T[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) pt[a] = T[4 + a];
  }
  const float c = FULL ? d.c : 1.0f, s = FULL ? d.s : 0.0f;
  const long long first = slot * kScanRegQuota + threadIdx.x;
#pragma unroll 1
  for (int trip = 0; trip < kScanRegTrips; ++trip) {
    const long long j = first + (long long)trip * kScanRegThreads;
    if (j >= d.n_strided) break;
    const long long i = j * d.stride;  // (< n)
    const float pc[3] = {d.points[3 * i], d.points[3 * i + 1], d.points[3 * i + 2]};
    const float range2 = (pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2];
    if (!(range2 >= d.min_range2 && range2 <= d.max_range2)) continue;
    ++n_cand;
    float q[3];
    quat_rotate(pq, pc, q);
    const float pm[3] = {(c * q[0] - s * q[1]) + pt[0], (s * q[0] + c * q[1]) + pt[1], q[2] + pt[2]};
    bool any = false;
#pragma unroll 1
    for (int m = 0; m < d.n_submaps; ++m) {
      const ScanMapSubmapDev& sm = d.submaps[m];  // (uniform: scalar loads)
      float pos[3];
      // rigid_apply and (below) interp_neighbours in this kernel's own lines: through rigid_apply the cost-only
      // instantiations came out a different instruction stream, through interp_neighbours their 24 gathers became flat
      // loads (16 of them with the table taken by value first)
      quat_rotate(sm.q_sm, pm, pos);
#pragma unroll
      for (int a = 0; a < 3; ++a) pos[a] = pos[a] + sm.t_sm[a];
      // the query kernel's rule: a block coordinate outside (-2^30, 2^30) -- every non-finite point -- is skipped
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) ok = ok && fabsf(pos[a] * sm.block_size_inv) < 1073741824.0f;
      if (!ok) continue;
      int blk[3], vox[3];
      float dl[3];
      interp_base<VPS>(sm, pos, blk, vox, dl);
      // the low neighbour's block outside the table's box: neighbour 0 is absent whatever the table holds
      const int3 lo = sm.lut_min, dim = sm.lut_dim;
      if ((unsigned)(blk[0] - lo.x) >= (unsigned)dim.x || (unsigned)(blk[1] - lo.y) >= (unsigned)dim.y ||
          (unsigned)(blk[2] - lo.z) >= (unsigned)dim.z)
        continue;
      // the 8 neighbours (k: x = bit 2, y = bit 1, z = bit 0): the addresses first, then the gathers together
      size_t at[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int off[3] = {(k >> 2) & 1, (k >> 1) & 1, k & 1};
        int nb[3], nv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          nb[a] = blk[a];
          nv[a] = vox[a] + off[a];
          if (nv[a] >= VPS) {
            nb[a]++;
            nv[a] -= VPS;
          }
        }
        const int bs = interp_slot(sm, nb[0], nb[1], nb[2]);
        ok = ok && bs >= 0;
        at[k] = (size_t)(bs >= 0 ? bs : 0) * VOX + (size_t)(nv[0] + VPS * (nv[1] + VPS * nv[2]));
      }
      if (!ok) continue;
      float x[8];
      const float* __restrict__ val = sm.val;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        x[k] = val[at[k]];
        if (TSDF)
          ok = ok && interp_valid(static_cast<const float*>(sm.vld)[at[k]]);
        else
          ok = ok && interp_valid(static_cast<const uint8_t*>(sm.vld)[at[k]]);
      }
      if (!ok) continue;
      const float r = interp_trilinear(x, dl);
      if (!(fabsf(r) < d.max_abs_distance)) continue;
      ++n_terms;
      any = true;
      // Huber in f64, arithmetic alone
      const double rd = (double)r, ar = fabs(rd), a = d.huber;
      double w = 1.0, rho = rd * rd;
      if (!(ar <= a)) {
        w = a / ar;
        rho = (2.0 * a) * ar - a * a;
      }
      acc.s[0] += rho;
      if constexpr (FULL) {
        float gl[3], gs[3], J[4];
        interp_trilinear_gradient(x, dl, gl);
#pragma unroll
        for (int a3 = 0; a3 < 3; ++a3) gs[a3] = gl[a3] * sm.voxel_size_inv;
        quat_rotate(sm.q_ms, gs, J);  // J[0..2] = g_M
        J[3] = J[0] * ((-s) * q[0] - c * q[1]) + J[1] * (c * q[0] - s * q[1]);
        const double Jd[4] = {(double)J[0], (double)J[1], (double)J[2], (double)J[3]};
        const double wr = w * rd;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc.s[1 + k] += Jd[k] * wr;
        int e = 5;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int l = k; l < 4; ++l) acc.s[e++] += (w * Jd[k]) * Jd[l];
      }
    }
    if (any) ++n_valid;
  }
  acc.n[0] = n_terms;
  acc.n[1] = n_valid;
  acc.n[2] = n_cand;
  scan_map_block_fold<kScanRegThreads / 64>(acc, static_cast<ScanMapSums<NS>*>(d.partials) + blockIdx.x);
}

// workgroup p: partials [p groups, (p + 1) groups) -> out[p]; partial b to thread b % 256, added to 0.0 in ascending b
template <int NS>
__global__ __launch_bounds__(kScanRegFold) void scan_map_fold_kernel(const ScanMapSums<NS>* __restrict__ partials, int groups,
                                                                    ScanMapSums<NS>* __restrict__ out) {
  ScanMapSums<NS> acc;
#pragma unroll
  for (int k = 0; k < NS; ++k) acc.s[k] = 0.0;
#pragma unroll
  for (int k = 0; k < kScanMapCounts; ++k) acc.n[k] = 0;
  const ScanMapSums<NS>* __restrict__ mine = partials + (size_t)blockIdx.x * (size_t)groups;
  for (int b = threadIdx.x; b < groups; b += kScanRegFold) {
    const ScanMapSums<NS> p = mine[b];
#pragma unroll
    for (int k = 0; k < NS; ++k) acc.s[k] += p.s[k];
#pragma unroll
    for (int k = 0; k < kScanMapCounts; ++k) acc.n[k] += p.n[k];
  }
  scan_map_block_fold<kScanRegFold / 64>(acc, out + blockIdx.x);
}

using ScanMapTotals = ScanMapSums<kScanRegSums>;
using ScanMapScore = ScanMapSums<1>;

template <bool FULL>
void launch_scan_map_eval(hipStream_t st, int vps, bool tsdf, unsigned blocks, const ScanMapDev& d) {
  void (*k)(ScanMapDev) = vps == 16 ? (tsdf ? scan_map_eval_kernel<16, true, FULL> : scan_map_eval_kernel<16, false, FULL>)
                                    : (tsdf ? scan_map_eval_kernel<8, true, FULL> : scan_map_eval_kernel<8, false, FULL>);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(kScanRegThreads), 0, st, d);
}

}  // namespace vgx

using namespace vgx;

namespace {

const char* map_config_error(const vgx_scan_map_config& c) {
  if (c.layer != VGX_EVAL_LAYER_ESDF && c.layer != VGX_EVAL_LAYER_TSDF) return "layer is neither ESDF nor TSDF";
  if (!(c.huber_delta_m > 0.0f)) return "huber_delta_m must be positive (+inf: no loss)";
  if (c.score_point_stride < 1) return "score_point_stride < 1";
  return nullptr;
}

int64_t map_groups(int64_t n, int32_t stride) {
  const int64_t strided = (n + stride - 1) / stride;
  return (strided + kScanRegQuota - 1) / kScanRegQuota;
}

// R->mu and ctx->mu held: every listed submap's chosen layer is resident, and the device table says where it lies now
int map_table(const char* fn, vgx_scan_registration R) {
  vgx_ctx ctx = R->ctx;
  const bool tsdf = R->map_cfg.layer == VGX_EVAL_LAYER_TSDF;
  const size_t n = R->map_submaps.size();
  bool changed = !R->d_map_desc.p;
  for (size_t k = 0; k < n; ++k) {
    vgx_submap sm = R->map_submaps[k];
    const float* val = tsdf ? sm->d_tsdf_distance.get() : sm->d_esdf_distance.get();
    const void* vld = tsdf ? (const void*)sm->d_tsdf_weight.get() : (const void*)sm->d_esdf_observed.get();
    if (sm->n_blocks > 0 && !(val && vld))
      return reg_fail(ctx, fn, "submap " + std::to_string(k) + ": " + (tsdf ? "TSDF" : "ESDF") +
                                   " layer not resident (released, or never generated)");
    ScanMapSubmapDev& e = R->map_desc[k];
    changed = changed || e.val != val || e.vld != vld || e.lut != sm->d_lut.get();
    e.val = val;
    e.vld = vld;
    static_cast<LayerTable&>(e) = submap_table(sm);
  }
  if (changed) {
    const size_t bytes = n * sizeof(ScanMapSubmapDev);
    if (bytes > R->d_map_desc.bytes) {
      const hipError_t e = R->d_map_desc.alloc(bytes);
      if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration: allocating the submap table");
    }
    VGX_HIP(ctx, hipMemcpyAsync(R->d_map_desc.p, R->map_desc.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  return VGX_OK;
}

void map_descriptor_common(vgx_scan_registration R, const float* d_points, int64_t n, int32_t stride, ScanMapDev* d) {
  *d = ScanMapDev{};
  d->submaps = R->d_map_desc.as<ScanMapSubmapDev>();
  d->n_submaps = (int32_t)R->map_submaps.size();
  d->stride = stride;
  d->points = d_points;
  d->n_strided = (n + stride - 1) / stride;
  d->min_range2 = R->cfg.min_range_m * R->cfg.min_range_m;
  d->max_range2 = R->cfg.max_range_m * R->cfg.max_range_m;
  d->max_abs_distance = R->cfg.max_abs_distance_m;
  d->huber = (double)R->map_cfg.huber_delta_m;
}

int map_reserve(vgx_scan_registration R, size_t partial_bytes, size_t out_bytes, size_t stage_bytes) {
  vgx_ctx ctx = R->ctx;
  // (every call on this route ends in a synchronisation: nothing queued reads the arrays now)
  hipError_t e = R->d_map_partials.reserve(partial_bytes, 64 * sizeof(ScanMapTotals), true);
  if (e == hipSuccess) e = R->d_map_out.reserve(out_bytes, sizeof(ScanMapTotals));
  if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration: allocating the map partials");
  e = R->h_map_stage.reserve(std::max(stage_bytes, sizeof(ScanMapTotals)));
  if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration: allocating the pinned stage");
  return VGX_OK;
}

// One evaluation: R->mu and ctx->mu held, the device set, map_table done.  `tot` receives the loop's view of the totals
// (n_valid = n_points_valid), *n_terms the third count.
int map_evaluate_locked(vgx_scan_registration R, const float* d_points, int64_t n, const float T[7], const double delta[4],
                        ScanRegPartial* tot, int64_t* n_terms) {
  vgx_ctx ctx = R->ctx;
  hipStream_t st = ctx->stream;
  std::memset(tot, 0, sizeof(*tot));
  *n_terms = 0;
  if (n <= 0) return VGX_OK;
  const int64_t groups = map_groups(n, R->cfg.point_stride);
  int rc = map_reserve(R, (size_t)groups * sizeof(ScanMapTotals), sizeof(ScanMapTotals), sizeof(ScanMapTotals));
  if (rc != VGX_OK) return rc;
  ScanMapDev d;
  map_descriptor_common(R, d_points, n, R->cfg.point_stride, &d);
  for (int k = 0; k < 4; ++k) d.q[k] = T[k];
  for (int a = 0; a < 3; ++a) d.t[a] = (float)((double)T[4 + a] + delta[a]);
  d.c = (float)std::cos(delta[3]);
  d.s = (float)std::sin(delta[3]);
  d.partials = R->d_map_partials.p;
  launch_scan_map_eval<true>(st, R->map_vps, R->map_cfg.layer == VGX_EVAL_LAYER_TSDF, (unsigned)groups, d);
  VGX_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(scan_map_fold_kernel<kScanRegSums>, dim3(1), dim3(kScanRegFold), 0, st, R->d_map_partials.as<ScanMapTotals>(),
                     (int)groups, R->d_map_out.as<ScanMapTotals>());
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, hipMemcpyAsync(R->h_map_stage.p, R->d_map_out.p, sizeof(ScanMapTotals), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  const ScanMapTotals& h = *R->h_map_stage.as<ScanMapTotals>();
  for (int k = 0; k < kScanRegSums; ++k) tot->s[k] = h.s[k];
  *n_terms = h.n[0];
  tot->n_valid = h.n[1];
  tot->n_candidates = h.n[2];
  return VGX_OK;
}

// All poses' costs and counts: R->mu and ctx->mu held, the device set, map_table done.  `scores` [n_poses].
int map_score_locked(vgx_scan_registration R, const float* d_points, int64_t n, int32_t n_poses, const float* T,
                     std::vector<ScanMapScore>* scores) {
  vgx_ctx ctx = R->ctx;
  hipStream_t st = ctx->stream;
  scores->assign((size_t)n_poses, ScanMapScore{});
  if (n <= 0 || n_poses == 0) return VGX_OK;
  const int32_t stride = R->map_cfg.score_point_stride;
  const int64_t groups = map_groups(n, stride);
  const size_t np = (size_t)n_poses;
  int rc = map_reserve(R, (size_t)groups * np * sizeof(ScanMapScore), np * sizeof(ScanMapScore), np * sizeof(ScanMapScore));
  if (rc != VGX_OK) return rc;
  if (np * 28 > R->d_map_poses.bytes) {
    const hipError_t e = R->d_map_poses.reserve(np * 28, 0, true);
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration: allocating the pose table");
  }
  // the table as the evaluation at delta = 0 sees a pose: t' = (float)((double)t + 0.0)
  float* up = R->h_map_stage.as<float>();
  for (size_t m = 0; m < np; ++m) {
    for (int k = 0; k < 4; ++k) up[7 * m + k] = T[7 * m + k];
    for (int a = 0; a < 3; ++a) up[7 * m + 4 + a] = (float)((double)T[7 * m + 4 + a] + 0.0);
  }
  VGX_HIP(ctx, hipMemcpyAsync(R->d_map_poses.p, up, np * 28, hipMemcpyHostToDevice, st));
  ScanMapDev d;
  map_descriptor_common(R, d_points, n, stride, &d);
  d.poses = R->d_map_poses.as<float>();
  d.groups = (int32_t)groups;
  d.partials = R->d_map_partials.p;
  launch_scan_map_eval<false>(st, R->map_vps, R->map_cfg.layer == VGX_EVAL_LAYER_TSDF, (unsigned)(groups * n_poses), d);
  VGX_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(scan_map_fold_kernel<1>, dim3((unsigned)n_poses), dim3(kScanRegFold), 0, st, R->d_map_partials.as<ScanMapScore>(),
                     (int)groups, R->d_map_out.as<ScanMapScore>());
  VGX_HIP(ctx, hipGetLastError());
  // (the upload above has left the stage by the time this copy runs: one stream)
  VGX_HIP(ctx, hipMemcpyAsync(R->h_map_stage.p, R->d_map_out.p, np * sizeof(ScanMapScore), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  std::memcpy(scores->data(), R->h_map_stage.p, np * sizeof(ScanMapScore));
  return VGX_OK;
}

// what the map calls refuse alike once R->mu is held: no map, no points, a launch too large.  `n_poses` < 0: one evaluation.
int map_source(const char* fn, vgx_scan_registration R, int32_t n_poses, const float** d_points, int64_t* n,
               std::unique_lock<std::mutex>* scan_lock) {
  vgx_ctx ctx = R->ctx;
  if (R->map_submaps.empty()) return reg_fail(ctx, fn, "no map set");
  const int rc = reg_points(fn, R, d_points, n, scan_lock);
  if (rc != VGX_OK) return rc;
  const int64_t groups = map_groups(*n, n_poses < 0 ? R->cfg.point_stride : R->map_cfg.score_point_stride);
  if (groups > 0x7fffffffll || (n_poses > 0 && groups * (int64_t)n_poses > 0x7fffffffll))
    return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": too many points (times poses) for one launch");
  return VGX_OK;
}

int map_check_poses(const char* fn, vgx_ctx ctx, int32_t n_poses, const float* T, const char* what) {
  for (int32_t m = 0; m < n_poses; ++m)
    if (const char* why = reg_pose_error(T + 7 * (size_t)m))
      return reg_fail(ctx, fn, std::string(what) + " " + std::to_string(m) + " " + why);
  return VGX_OK;
}

int map_options(const char* fn, vgx_ctx ctx, const vgx_pose_graph_options* options, vgx_pose_graph_options* opt) {
  vgx_pose_graph_options_default(opt);
  if (options) *opt = *options;
  if (!(opt->initial_trust_region_radius > 0.0)) return reg_fail(ctx, fn, "initial_trust_region_radius must be positive");
  return VGX_OK;
}

int map_refine_locked(vgx_scan_registration R, const float* d_points, int64_t n, const float T[7], const vgx_pose_graph_options& opt,
                      float T_refined[7], double delta_out[4], vgx_scan_registration_summary* summary) {
  return reg_refine_loop(
      R, T, opt,
      [&](const double x[4], ScanRegPartial* tot) {
        int64_t n_terms;
        return map_evaluate_locked(R, d_points, n, T, x, tot, &n_terms);
      },
      T_refined, delta_out, summary);
}

}  // namespace

void vgx::scan_map_release(vgx_scan_registration R) {
  std::vector<vgx_submap> orphans;
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    for (vgx_submap sm : R->map_submaps)
      if (--sm->users == 0 && sm->destroy_requested) orphans.push_back(sm);
  }
  R->map_submaps.clear();
  R->map_desc.clear();
  R->map_vps = 0;
  for (vgx_submap sm : orphans) (void)vgx_submap_destroy(sm);
}

extern "C" {

void vgx_scan_map_config_default(vgx_scan_map_config* cfg) {
  if (!cfg) return;
  cfg->layer = VGX_EVAL_LAYER_ESDF;
  cfg->huber_delta_m = std::numeric_limits<float>::infinity();
  cfg->score_point_stride = 1;
  cfg->reserved = 0;
}

int vgx_scan_registration_set_map(vgx_scan_registration R, const vgx_scan_map_config* cfg, int32_t n_submaps, const vgx_submap* submaps,
                                  const float* T_M_S) {
  const char* fn = "vgx_scan_registration_set_map";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  vgx_scan_map_config c;
  vgx_scan_map_config_default(&c);
  if (cfg) c = *cfg;
  if (const char* why = map_config_error(c)) return reg_fail(ctx, fn, why);
  if (n_submaps < 0 || n_submaps > kScanMapMaxSubmaps) return reg_fail(ctx, fn, "n_submaps < 0 or > 64");
  if (n_submaps > 0 && (!submaps || !T_M_S)) return reg_fail(ctx, fn, "NULL submaps or poses");
  std::vector<ScanMapSubmapDev> desc((size_t)n_submaps);
  for (int32_t k = 0; k < n_submaps; ++k) {
    vgx_submap sm = submaps[k];
    if (!sm) return reg_fail(ctx, fn, "NULL submap " + std::to_string(k));
    if (sm->ctx != ctx) return reg_fail(ctx, fn, "submap " + std::to_string(k) + " belongs to another context");
    if (sm->vps != 8 && sm->vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": voxels_per_side not 8 or 16");
    if (sm->vps != submaps[0]->vps) return reg_fail(ctx, fn, "submaps of different voxels_per_side");
  }
  int rc = map_check_poses(fn, ctx, n_submaps, T_M_S, "the pose of submap");
  if (rc != VGX_OK) return rc;
  for (int32_t k = 0; k < n_submaps; ++k) {
    const float* T = T_M_S + 7 * (size_t)k;
    ScanMapSubmapDev& e = desc[(size_t)k];
    e = ScanMapSubmapDev{};  // (the block table and the layer pointers: map_table, at every evaluation)
    for (int i = 0; i < 4; ++i) e.q_ms[i] = T[i];
    inverse_pose(T, T + 4, e.q_sm, e.t_sm);  // T_S_M, once in f32
  }
  std::lock_guard<std::mutex> lk(R->mu);
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    for (int32_t k = 0; k < n_submaps; ++k) ++submaps[k]->users;
  }
  scan_map_release(R);  // (after the new counts: a submap in both lists stays)
  R->map_cfg = c;
  R->map_submaps.assign(submaps, submaps + n_submaps);
  R->map_desc.swap(desc);
  R->map_vps = n_submaps > 0 ? submaps[0]->vps : 0;
  R->d_map_desc.release();  // (nothing queued reads it: every call ends in a synchronisation); uploaded by the next evaluation
  return VGX_OK;
}

int vgx_scan_registration_evaluate_map(vgx_scan_registration R, const float T[7], const double delta[4], double out[15],
                                       int64_t* n_terms, int64_t* n_points_valid, int64_t* n_candidates) {
  const char* fn = "vgx_scan_registration_evaluate_map";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  if (!T || !delta || !out) return reg_fail(ctx, fn, "NULL prior, delta or output");
  if (const char* why = reg_pose_error(T)) return reg_fail(ctx, fn, std::string("the prior ") + why);
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(delta[k])) return reg_fail(ctx, fn, "delta is not finite");
  std::lock_guard<std::mutex> lk(R->mu);
  const float* d_points = nullptr;
  int64_t n = 0;
  std::unique_lock<std::mutex> scan_lock;
  int rc = map_source(fn, R, -1, &d_points, &n, &scan_lock);
  if (rc != VGX_OK) return rc;
  ScanRegPartial tot;
  int64_t terms = 0;
  {
    std::lock_guard<std::mutex> ctx_lk(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    rc = map_table(fn, R);
    if (rc == VGX_OK) rc = map_evaluate_locked(R, d_points, n, T, delta, &tot, &terms);
    if (rc != VGX_OK) return rc;
  }
  for (int k = 0; k < kScanRegSums; ++k) out[k] = tot.s[k];
  if (n_terms) *n_terms = terms;
  if (n_points_valid) *n_points_valid = tot.n_valid;
  if (n_candidates) *n_candidates = tot.n_candidates;
  return VGX_OK;
}

int vgx_scan_registration_refine_map(vgx_scan_registration R, const float T[7], const vgx_pose_graph_options* options,
                                     float T_refined[7], double delta_out[4], vgx_scan_registration_summary* summary) {
  const char* fn = "vgx_scan_registration_refine_map";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  if (!T || !T_refined || !delta_out) return reg_fail(ctx, fn, "NULL prior, T_refined or delta");
  if (const char* why = reg_pose_error(T)) return reg_fail(ctx, fn, std::string("the prior ") + why);
  vgx_pose_graph_options opt;
  int rc = map_options(fn, ctx, options, &opt);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> lk(R->mu);
  const float* d_points = nullptr;
  int64_t n = 0;
  std::unique_lock<std::mutex> scan_lock;
  rc = map_source(fn, R, -1, &d_points, &n, &scan_lock);
  if (rc != VGX_OK) return rc;
  // the whole solve under the registration side's lock: every evaluation sees the layers the first one saw
  std::lock_guard<std::mutex> ctx_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  rc = map_table(fn, R);
  if (rc != VGX_OK) return rc;
  return map_refine_locked(R, d_points, n, T, opt, T_refined, delta_out, summary);
}

int vgx_scan_registration_score_poses(vgx_scan_registration R, int32_t n_poses, const float* T, double* cost, int64_t* n_terms,
                                      int64_t* n_points_valid, int64_t* n_candidates) {
  const char* fn = "vgx_scan_registration_score_poses";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  if (n_poses < 0 || (n_poses > 0 && !T)) return reg_fail(ctx, fn, "n_poses < 0 or NULL poses");
  int rc = map_check_poses(fn, ctx, n_poses, T, "pose");
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> lk(R->mu);
  const float* d_points = nullptr;
  int64_t n = 0;
  std::unique_lock<std::mutex> scan_lock;
  rc = map_source(fn, R, n_poses, &d_points, &n, &scan_lock);
  if (rc != VGX_OK) return rc;
  std::vector<ScanMapScore> scores;
  {
    std::lock_guard<std::mutex> ctx_lk(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    rc = map_table(fn, R);
    if (rc == VGX_OK) rc = map_score_locked(R, d_points, n, n_poses, T, &scores);
    if (rc != VGX_OK) return rc;
  }
  for (int32_t m = 0; m < n_poses; ++m) {
    const ScanMapScore& s = scores[(size_t)m];
    if (cost) cost[m] = 0.5 * s.s[0];
    if (n_terms) n_terms[m] = s.n[0];
    if (n_points_valid) n_points_valid[m] = s.n[1];
    if (n_candidates) n_candidates[m] = s.n[2];
  }
  return VGX_OK;
}

int vgx_scan_registration_localize(vgx_scan_registration R, int32_t n_poses, const float* T, const vgx_pose_graph_options* options,
                                   int32_t* best_index, float T_refined[7], double delta_out[4],
                                   vgx_scan_registration_summary* summary) {
  const char* fn = "vgx_scan_registration_localize";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  if (n_poses < 0 || (n_poses > 0 && !T)) return reg_fail(ctx, fn, "n_poses < 0 or NULL poses");
  if (!best_index || !T_refined || !delta_out) return reg_fail(ctx, fn, "NULL best_index, T_refined or delta");
  int rc = map_check_poses(fn, ctx, n_poses, T, "pose");
  if (rc != VGX_OK) return rc;
  vgx_pose_graph_options opt;
  rc = map_options(fn, ctx, options, &opt);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> lk(R->mu);
  const float* d_points = nullptr;
  int64_t n = 0;
  std::unique_lock<std::mutex> scan_lock;
  rc = map_source(fn, R, n_poses, &d_points, &n, &scan_lock);
  if (rc != VGX_OK) return rc;
  if (map_groups(n, R->cfg.point_stride) > 0x7fffffffll)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": too many points for one launch");
  std::lock_guard<std::mutex> ctx_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  rc = map_table(fn, R);
  if (rc != VGX_OK) return rc;
  std::vector<ScanMapScore> scores;
  rc = map_score_locked(R, d_points, n, n_poses, T, &scores);
  if (rc != VGX_OK) return rc;
  int32_t best = -1;
  double best_score = 0.0;
  for (int32_t m = 0; m < n_poses; ++m) {
    const ScanMapScore& s = scores[(size_t)m];
    if (!(s.n[2] > 0 && (double)s.n[1] / (double)s.n[2] >= (double)R->cfg.min_valid_ratio)) continue;
    const double score = (0.5 * s.s[0]) / (double)s.n[0];
    if (best < 0 || score < best_score) {
      best = m;
      best_score = score;
    }
  }
  *best_index = best;
  if (best < 0) {
    vgx_scan_registration_summary S;
    std::memset(&S, 0, sizeof(S));
    S.termination_type = VGX_FAILURE;
    S.termination_reason = VGX_TERMINATION_TOO_FEW_POINTS;
    if (n_poses > 0)
      for (int k = 0; k < 7; ++k) T_refined[k] = T[k];
    for (int k = 0; k < 4; ++k) delta_out[k] = 0.0;
    R->history.clear();
    if (summary) *summary = S;
    return VGX_OK;
  }
  return map_refine_locked(R, d_points, n, T + 7 * (size_t)best, opt, T_refined, delta_out, summary);
}

}  // extern "C"
