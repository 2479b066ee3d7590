// Scan-to-map registration (include/voxgraph_amd.h, "Scan-to-map registration"): a scan's sensor pose
// refined against the active TSDF layer by point-to-implicit-surface Gauss-Newton over a 4-DoF correction.  The
// formulation and the order contract are stated in the header; tests/scan_registration_ref.py restates every bit.
//
//   1. scan_reg_eval_kernel: candidate j (point j * stride) to workgroup j / 1024, thread (j % 1024) % 256, trip
//      (j % 1024) / 256.  Per point one rotation, one block-table lookup per neighbour and 8 dependent 8-byte gathers
//      of {distance, weight}; the residual and the exact gradient of the interpolant from those 8 voxels; 15 f64 sums
//      and two counts per thread, folded by the wave tree and the waves in order into one partial per workgroup.
//   2. scan_reg_fold_kernel: one workgroup of 256 threads folds the partials in workgroup order.
// One D2H copy of 136 bytes into the handle's pinned stage and one synchronisation per evaluation.  No float atomics.
// The handle, the partition's constants and the trust-region loop live in vgx_scan_reg_internal.h: scan localisation
// (vgx_scan_localize.hip) shares them.
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "vgx_internal.h"
#include "vgx_interp.h"
#include "vgx_query_kernel.h"
#include "vgx_scan_reg_internal.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

struct ScanRegDev : LayerTable {  // (the live layer's)
  const unsigned long long* voxels;  // [blocks][vps^3] {distance (lo), weight (hi)}
  const float* points;               // [n][3] sensor frame
  long long n_strided;               // candidates by stride alone: ceil(n / stride)
  int32_t stride;
  float q[4], t[3];                  // the prior's rotation; t' = (float)((double)t_prior + delta)
  float c, s;                        // (float)cos / sin(delta yaw)
  float min_range2, max_range2, max_abs_distance;
  ScanRegPartial* partials;          // [workgroups]
};

__device__ __forceinline__ void scan_reg_wave_fold(double (&v)[kScanRegSums], long long& a, long long& b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < kScanRegSums; ++k) v[k] += __shfl_down(v[k], o);
    a += __shfl_down(a, o);
    b += __shfl_down(b, o);
  }
}

// lane 0 of every wave holds its wave's sums: the waves in order, by thread 0 -> out
template <int WAVES>
__device__ __forceinline__ void scan_reg_block_fold(double (&v)[kScanRegSums], long long n_valid, long long n_cand,
                                                    ScanRegPartial* out) {
  __shared__ double sh[WAVES][kScanRegSums];
  __shared__ long long sh_n[WAVES][2];
  scan_reg_wave_fold(v, n_valid, n_cand);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kScanRegSums; ++k) sh[w][k] = v[k];
    sh_n[w][0] = n_valid;
    sh_n[w][1] = n_cand;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScanRegPartial p;
#pragma unroll
    for (int k = 0; k < kScanRegSums; ++k) p.s[k] = sh[0][k];
    p.n_valid = sh_n[0][0];
    p.n_candidates = sh_n[0][1];
    for (int i = 1; i < WAVES; ++i) {  // the waves in order
#pragma unroll
      for (int k = 0; k < kScanRegSums; ++k) p.s[k] += sh[i][k];
      p.n_valid += sh_n[i][0];
      p.n_candidates += sh_n[i][1];
    }
    *out = p;
  }
}

template <int VPS>
__global__ __launch_bounds__(kScanRegThreads) void scan_reg_eval_kernel(ScanRegDev d) {
  double acc[kScanRegSums];
#pragma unroll
  for (int k = 0; k < kScanRegSums; ++k) acc[k] = 0.0;
  long long n_valid = 0, n_cand = 0;
  const long long first = (long long)blockIdx.x * kScanRegQuota + threadIdx.x;
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
    quat_rotate(d.q, pc, q);
    const float pos[3] = {(d.c * q[0] - d.s * q[1]) + d.t[0], (d.s * q[0] + d.c * q[1]) + d.t[1], q[2] + d.t[2]};
    // the query kernel's rule: a block coordinate outside (-2^30, 2^30) -- every non-finite point -- is skipped
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && fabsf(pos[a] * d.block_size_inv) < 1073741824.0f;
    if (!ok) continue;
    int blk[3], vox[3];
    float dl[3];
    interp_base<VPS>(d, pos, blk, vox, dl);
    // the 8 neighbours' addresses first, then the gathers together
    size_t at[8];
    if (!interp_neighbours<VPS>(d, blk, vox, at)) continue;
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const unsigned long long v = d.voxels[at[k]];
      x[k] = __uint_as_float((unsigned int)(v & 0xffffffffull));
      ok = ok && interp_valid(__uint_as_float((unsigned int)(v >> 32)));
    }
    if (!ok) continue;
    const float r = interp_trilinear(x, dl);
    if (!(fabsf(r) < d.max_abs_distance)) continue;
    float gl[3];
    interp_trilinear_gradient(x, dl, gl);
    float J[4];
#pragma unroll
    for (int a = 0; a < 3; ++a) J[a] = gl[a] * d.voxel_size_inv;
    J[3] = J[0] * ((-d.s) * q[0] - d.c * q[1]) + J[1] * (d.c * q[0] - d.s * q[1]);
    ++n_valid;
    const double rd = (double)r;
    const double Jd[4] = {(double)J[0], (double)J[1], (double)J[2], (double)J[3]};
    acc[0] += rd * rd;
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[1 + k] += Jd[k] * rd;
    int e = 5;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int l = k; l < 4; ++l) acc[e++] += Jd[k] * Jd[l];
  }
  scan_reg_block_fold<kScanRegThreads / 64>(acc, n_valid, n_cand, d.partials + blockIdx.x);
}

__global__ __launch_bounds__(kScanRegFold) void scan_reg_fold_kernel(const ScanRegPartial* __restrict__ partials, int n_partials,
                                                                    ScanRegPartial* __restrict__ out) {
  double acc[kScanRegSums];
#pragma unroll
  for (int k = 0; k < kScanRegSums; ++k) acc[k] = 0.0;
  long long n_valid = 0, n_cand = 0;
  for (int b = threadIdx.x; b < n_partials; b += kScanRegFold) {
    const ScanRegPartial p = partials[b];
#pragma unroll
    for (int k = 0; k < kScanRegSums; ++k) acc[k] += p.s[k];
    n_valid += p.n_valid;
    n_cand += p.n_candidates;
  }
  scan_reg_block_fold<kScanRegFold / 64>(acc, n_valid, n_cand, out);
}

}  // namespace vgx

using namespace vgx;

namespace {

const char* config_error(const vgx_scan_registration_config& c) {
  if (c.point_stride < 1) return "point_stride < 1";
  if (!(c.max_abs_distance_m > 0.0f) || !std::isfinite(c.max_abs_distance_m)) return "max_abs_distance_m must be positive and finite (it has no default)";
  if (std::isnan(c.min_range_m) || std::isnan(c.max_range_m) || c.min_range_m > c.max_range_m) return "min_range_m > max_range_m, or a NaN range";
  if (!std::isfinite(c.min_valid_ratio)) return "min_valid_ratio is not finite";
  return nullptr;
}

// what evaluate and refine refuse alike, before any lock
int reg_check(const char* fn, vgx_scan_registration R, vgx_tsdf_layer L, const float* T, const double* delta) {
  vgx_ctx ctx = R->ctx;
  if (!L || !T) return reg_fail(ctx, fn, "NULL layer or prior");
  if (L->ctx != ctx) return reg_fail(ctx, fn, "the layer belongs to another context");
  const PoseDefect bad = pose_defect(T);
  if (bad == kPoseNotFinite) return reg_fail(ctx, fn, "the prior is not finite");
  if (bad == kPoseNotUnit) return reg_fail(ctx, fn, "the prior's quaternion is not unit (| |q|^2 - 1 | > 1e-4)");
  if (delta)
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(delta[k])) return reg_fail(ctx, fn, "delta is not finite");
  if (L->dev.vps != 8 && L->dev.vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": voxels_per_side not 8 or 16");
  return VGX_OK;
}

}  // namespace

// the points of this evaluation, whatever their source (vgx_scan_reg_internal.h says which locks are held)
int vgx::reg_points(const char* fn, vgx_scan_registration R, const float** d_points, int64_t* n, std::unique_lock<std::mutex>* scan_lock) {
  vgx_ctx ctx = R->ctx;
  *d_points = nullptr;
  *n = 0;
  switch (R->source) {
    case vgx_scan_registration_s::kNone:
      return reg_fail(ctx, fn, "no points set");
    case vgx_scan_registration_s::kOwned:
      *d_points = R->d_points.as<float>();
      *n = R->n;
      break;
    case vgx_scan_registration_s::kDevice:
      *d_points = static_cast<const float*>(R->borrowed);
      *n = R->n;
      break;
    case vgx_scan_registration_s::kScan:
      *scan_lock = scan_borrow(R->scan, d_points, n);
      break;
  }
  return VGX_OK;
}

namespace {

// ... and the one launch they must fit
int reg_source(const char* fn, vgx_scan_registration R, const float** d_points, int64_t* n, std::unique_lock<std::mutex>* scan_lock) {
  vgx_ctx ctx = R->ctx;
  const int rc = reg_points(fn, R, d_points, n, scan_lock);
  if (rc != VGX_OK) return rc;
  const int64_t strided = (*n + R->cfg.point_stride - 1) / R->cfg.point_stride;
  if ((strided + kScanRegQuota - 1) / kScanRegQuota > 0x7fffffffll)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": too many points for one launch");
  return VGX_OK;
}

// One evaluation: R->mu and ctx->tsdf_mu held, the device set.  `tot` receives the totals.
int reg_evaluate_locked(vgx_scan_registration R, vgx_tsdf_layer L, const float* d_points, int64_t n, const float T[7],
                        const double delta[4], ScanRegPartial* tot) {
  vgx_ctx ctx = R->ctx;
  hipStream_t st = ctx->tsdf_stream;
  std::memset(tot, 0, sizeof(*tot));
  if (n <= 0) return VGX_OK;
  const int64_t strided = (n + R->cfg.point_stride - 1) / R->cfg.point_stride;
  const int64_t groups = (strided + kScanRegQuota - 1) / kScanRegQuota;
  if ((size_t)groups * sizeof(ScanRegPartial) > R->d_partials.bytes) {
    VGX_HIP(ctx, hipStreamSynchronize(st));  // (a queued fold may still read the old array)
    const hipError_t e = R->d_partials.reserve((size_t)groups * sizeof(ScanRegPartial), 64 * sizeof(ScanRegPartial), true);
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration: allocating the partials");
  }
  if (!R->d_out.p) {
    const hipError_t e = R->d_out.alloc(sizeof(ScanRegPartial));
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration: allocating the totals");
  }
  if (!R->h_out.p) {
    const hipError_t e = R->h_out.alloc(sizeof(ScanRegPartial));
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration: allocating the pinned stage");
  }
  const TsdfLayerDev& ld = L->dev;
  ScanRegDev d{};
  static_cast<LayerTable&>(d) = live_layer_table(L);
  d.voxels = ld.voxels;
  d.points = d_points;
  d.n_strided = strided;
  d.stride = R->cfg.point_stride;
  for (int k = 0; k < 4; ++k) d.q[k] = T[k];
  for (int a = 0; a < 3; ++a) d.t[a] = (float)((double)T[4 + a] + delta[a]);
  d.c = (float)std::cos(delta[3]);
  d.s = (float)std::sin(delta[3]);
  d.min_range2 = R->cfg.min_range_m * R->cfg.min_range_m;
  d.max_range2 = R->cfg.max_range_m * R->cfg.max_range_m;
  d.max_abs_distance = R->cfg.max_abs_distance_m;
  d.partials = R->d_partials.as<ScanRegPartial>();
  if (ld.vps == 16)
    hipLaunchKernelGGL(scan_reg_eval_kernel<16>, dim3((unsigned)groups), dim3(kScanRegThreads), 0, st, d);
  else
    hipLaunchKernelGGL(scan_reg_eval_kernel<8>, dim3((unsigned)groups), dim3(kScanRegThreads), 0, st, d);
  VGX_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(scan_reg_fold_kernel, dim3(1), dim3(kScanRegFold), 0, st, R->d_partials.as<ScanRegPartial>(), (int)groups,
                     R->d_out.as<ScanRegPartial>());
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, hipMemcpyAsync(R->h_out.p, R->d_out.p, sizeof(ScanRegPartial), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  *tot = *R->h_out.as<ScanRegPartial>();
  return VGX_OK;
}

}  // namespace

extern "C" {

void vgx_scan_registration_config_default(vgx_scan_registration_config* cfg) {
  if (!cfg) return;
  cfg->min_range_m = 0.0f;
  cfg->max_range_m = std::numeric_limits<float>::infinity();
  cfg->max_abs_distance_m = 0.0f;  // (no default: the caller states it)
  cfg->point_stride = 1;
  cfg->min_valid_ratio = 0.5f;
}

int vgx_scan_registration_create(vgx_ctx ctx, const vgx_scan_registration_config* cfg, vgx_scan_registration* out) {
  const char* fn = "vgx_scan_registration_create";
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL context or output");
  *out = nullptr;
  if (!cfg) return reg_fail(ctx, fn, "NULL config (max_abs_distance_m has no default)");
  if (const char* why = config_error(*cfg)) return reg_fail(ctx, fn, why);
  vgx_scan_registration R = new (std::nothrow) vgx_scan_registration_s;
  if (!R) return set_error(ctx, VGX_ERR_NOMEM, std::string(fn) + ": out of host memory");
  R->ctx = ctx;
  R->cfg = *cfg;
  *out = R;
  return VGX_OK;
}

int vgx_scan_registration_destroy(vgx_scan_registration R) {
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  {
    std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->tsdf_stream);
  }
  {
    std::lock_guard<std::mutex> lk(ctx->mu);  // (the map route's launches: every one ended in a synchronisation)
    (void)hipStreamSynchronize(ctx->stream);
  }
  scan_map_release(R);
  delete R;
  return VGX_OK;
}

int vgx_scan_registration_set_points(vgx_scan_registration R, const float* points, int64_t n) {
  const char* fn = "vgx_scan_registration_set_points";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  if (n < 0 || (n > 0 && !points)) return reg_fail(ctx, fn, "n < 0 or NULL points");
  std::lock_guard<std::mutex> lk(R->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->tsdf_stream;
  R->source = vgx_scan_registration_s::kNone;  // (what a failure below leaves)
  if (n > 0) {
    if ((size_t)n * 12 > R->d_points.bytes) {
      const hipError_t e = R->d_points.reserve((size_t)n * 12, 0, true);
      if (e != hipSuccess) return alloc_error(ctx, e, "vgx_scan_registration_set_points: allocating the points");
    }
    // (every evaluation ends with a synchronisation: nothing queued reads the array now)
    VGX_HIP(ctx, hipMemcpyAsync(R->d_points.p, points, (size_t)n * 12, hipMemcpyHostToDevice, st));
    VGX_HIP(ctx, hipStreamSynchronize(st));
  }
  R->n = n;
  R->borrowed = nullptr;
  R->scan = nullptr;
  R->source = vgx_scan_registration_s::kOwned;
  return VGX_OK;
}

int vgx_scan_registration_set_points_device(vgx_scan_registration R, const void* d_points, int64_t n) {
  if (!R) return VGX_ERR_INVALID;
  if (n < 0 || (n > 0 && !d_points)) return reg_fail(R->ctx, "vgx_scan_registration_set_points_device", "n < 0 or NULL points");
  std::lock_guard<std::mutex> lk(R->mu);
  R->n = n;
  R->borrowed = d_points;
  R->scan = nullptr;
  R->source = vgx_scan_registration_s::kDevice;
  return VGX_OK;
}

int vgx_scan_registration_set_scan(vgx_scan_registration R, vgx_scan scan) {
  if (!R) return VGX_ERR_INVALID;
  const char* fn = "vgx_scan_registration_set_scan";
  if (!scan) return reg_fail(R->ctx, fn, "NULL scan");
  if (scan_context(scan) != R->ctx) return reg_fail(R->ctx, fn, "the scan belongs to another context");
  std::lock_guard<std::mutex> lk(R->mu);
  R->n = 0;
  R->borrowed = nullptr;
  R->scan = scan;
  R->source = vgx_scan_registration_s::kScan;
  return VGX_OK;
}

int vgx_scan_registration_evaluate(vgx_scan_registration R, vgx_tsdf_layer L, const float T[7], const double delta[4], double out[15],
                                   int64_t* n_valid, int64_t* n_candidates) {
  const char* fn = "vgx_scan_registration_evaluate";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  if (!delta || !out) return reg_fail(ctx, fn, "NULL delta or output");
  int rc = reg_check(fn, R, L, T, delta);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> lk(R->mu);
  const float* d_points = nullptr;
  int64_t n = 0;
  std::unique_lock<std::mutex> scan_lock;
  rc = reg_source(fn, R, &d_points, &n, &scan_lock);
  if (rc != VGX_OK) return rc;
  ScanRegPartial tot;
  {
    std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    rc = reg_evaluate_locked(R, L, d_points, n, T, delta, &tot);
    if (rc != VGX_OK) return rc;
  }
  for (int k = 0; k < kScanRegSums; ++k) out[k] = tot.s[k];
  if (n_valid) *n_valid = tot.n_valid;
  if (n_candidates) *n_candidates = tot.n_candidates;
  return VGX_OK;
}

int vgx_scan_registration_refine(vgx_scan_registration R, vgx_tsdf_layer L, const float T[7], const vgx_pose_graph_options* options,
                                 float T_refined[7], double delta_out[4], vgx_scan_registration_summary* summary) {
  const char* fn = "vgx_scan_registration_refine";
  if (!R) return VGX_ERR_INVALID;
  vgx_ctx ctx = R->ctx;
  if (!T_refined || !delta_out) return reg_fail(ctx, fn, "NULL T_refined or delta");
  int rc = reg_check(fn, R, L, T, nullptr);
  if (rc != VGX_OK) return rc;
  vgx_pose_graph_options opt;
  vgx_pose_graph_options_default(&opt);
  if (options) opt = *options;
  if (!(opt.initial_trust_region_radius > 0.0)) return reg_fail(ctx, fn, "initial_trust_region_radius must be positive");
  std::lock_guard<std::mutex> lk(R->mu);
  const float* d_points = nullptr;
  int64_t n = 0;
  std::unique_lock<std::mutex> scan_lock;
  rc = reg_source(fn, R, &d_points, &n, &scan_lock);
  if (rc != VGX_OK) return rc;
  // the whole solve under the TSDF side's lock: every evaluation sees the layer the first one saw
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  return reg_refine_loop(
      R, T, opt, [&](const double x[4], ScanRegPartial* tot) { return reg_evaluate_locked(R, L, d_points, n, T, x, tot); }, T_refined,
      delta_out, summary);
}

int vgx_scan_registration_history(vgx_scan_registration R, int32_t capacity, vgx_pose_graph_iteration* iterations, int32_t* n_iterations) {
  if (!R) return VGX_ERR_INVALID;
  if (capacity < 0 || (capacity > 0 && !iterations))
    return reg_fail(R->ctx, "vgx_scan_registration_history", "capacity < 0 or NULL iterations");
  std::lock_guard<std::mutex> lk(R->mu);
  if (n_iterations) *n_iterations = (int32_t)R->history.size();
  const size_t k = std::min(R->history.size(), (size_t)capacity);
  if (k) std::memcpy(iterations, R->history.data(), k * sizeof(vgx_pose_graph_iteration));
  return VGX_OK;
}

}  // extern "C"
