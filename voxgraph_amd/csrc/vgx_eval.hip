// Map evaluation on the device: voxblox::utils::evaluateLayersRmse(gt layer, test layer, mode, &details, &error_layer)
// [recalled] over the raw ESDF or TSDF layers of two finished submaps.  The rules and the fixed association of the f64
// sum are stated in include/voxgraph_amd.h (vgx_evaluate_layers_rmse); the passes and their measurement in DESIGN.md 12.
//
//   1. one thread per test block: its gt block through the gt submap's dense block table (eval_match_kernel)
//   2. only when error blocks are asked for: an exclusive scan of "has a gt block" gives each test block its error block
//   3. one workgroup per test block (eval_block_kernel): 4 consecutive voxels per thread per step (16-byte distance loads,
//      4-byte observed / weight loads), classified in registers; per-block partials (three int32 counts, max and min of
//      |e|, the f64 sum) and, if asked for, the error voxels
//   4. one 1024-thread workgroup (eval_fold_kernel) folds the partials in slot order and counts the gt blocks without a
//      test block; one D2H of the totals.
// No float atomics: every sum has one association, so the results are bit-identical run to run.
#include <algorithm>
#include <cmath>
#include <string>

#include "vgx_internal.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

struct EvalPartial {  // per test block, 32 B
  double sum;
  float max_abs, min_abs;
  int32_t n_eval, n_ign, n_non, pad;
};

struct EvalLut {
  const int32_t* lut;
  int3 mn, dim;
};

__device__ __forceinline__ int eval_lut_find(const EvalLut& L, const int32_t* bi) {
  const int rx = bi[0] - L.mn.x, ry = bi[1] - L.mn.y, rz = bi[2] - L.mn.z;
  if ((unsigned)rx >= (unsigned)L.dim.x || (unsigned)ry >= (unsigned)L.dim.y || (unsigned)rz >= (unsigned)L.dim.z) return -1;
  return L.lut[rx + L.dim.x * (ry + L.dim.y * rz)];
}

__global__ __launch_bounds__(256) void eval_match_kernel(const int32_t* __restrict__ test_bi, int n_test, EvalLut gt,
                                                         int32_t* __restrict__ gt_slot, int32_t* __restrict__ has) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_test) return;
  const int g = eval_lut_find(gt, test_bi + 3 * (size_t)t);
  gt_slot[t] = g;
  has[t] = g >= 0 ? 1 : 0;
}

// observed: ESDF observed != 0 (4 bytes of uint8 flags), TSDF weight > 1e-6f (4 floats)
template <bool TSDF>
__device__ __forceinline__ void eval_load_observed(const void* p, size_t at4, bool ok[4]) {
  if (TSDF) {
    const float4 w = reinterpret_cast<const float4*>(p)[at4];
    ok[0] = w.x > 1e-6f;
    ok[1] = w.y > 1e-6f;
    ok[2] = w.z > 1e-6f;
    ok[3] = w.w > 1e-6f;
  } else {
    const uint32_t o = reinterpret_cast<const uint32_t*>(p)[at4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = ((o >> (8 * j)) & 0xffu) != 0u;
  }
}

__device__ __forceinline__ void eval_wave_fold(double& s, float& mx, float& mn, int& a, int& b, int& c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_down(s, o);
    mx = fmaxf(mx, __shfl_down(mx, o));
    mn = fminf(mn, __shfl_down(mn, o));
    a += __shfl_down(a, o);
    b += __shfl_down(b, o);
    c += __shfl_down(c, o);
  }
}

// One workgroup of T = min(256, VOX / 4) threads per test block: voxel v = 4 (t + T k) + j belongs to thread t.
template <int VPS, bool TSDF>
__global__ __launch_bounds__(VPS == 16 ? 256 : 128) void eval_block_kernel(
    const int32_t* __restrict__ gt_slot, const float* __restrict__ gt_d, const void* __restrict__ gt_o,
    const float* __restrict__ test_d, const void* __restrict__ test_o, const int32_t* __restrict__ test_bi, int mode,
    EvalPartial* __restrict__ part, const int32_t* __restrict__ err_pos, float* __restrict__ err_d,
    uint8_t* __restrict__ err_set, int32_t* __restrict__ err_bi) {
  constexpr int VOX = VPS * VPS * VPS;
  constexpr int T = VPS == 16 ? 256 : 128;
  constexpr int K = VOX / (4 * T);
  constexpr int W = T / 64;
  __shared__ double s_sum[W];
  __shared__ float s_max[W], s_min[W];
  __shared__ int s_cnt[W][3];
  const int t = blockIdx.x;
  const int g = gt_slot[t];
  if (g < 0) {  // (uniform) no gt counterpart: every voxel non-overlapping, no error block
    if (threadIdx.x == 0) part[t] = EvalPartial{0.0, 0.0f, INFINITY, 0, 0, VOX, 0};
    return;
  }
  const bool ign_test = mode == VGX_EVAL_IGNORE_BEHIND_TEST || mode == VGX_EVAL_IGNORE_BEHIND_ALL;
  const bool ign_gt = mode == VGX_EVAL_IGNORE_BEHIND_GT || mode == VGX_EVAL_IGNORE_BEHIND_ALL;
  const size_t gbase4 = (size_t)g * (VOX / 4), tbase4 = (size_t)t * (VOX / 4);
  const size_t ebase4 = err_pos ? (size_t)err_pos[t] * (VOX / 4) : 0;
  double sum = 0.0;
  float mx = 0.0f, mn = INFINITY;
  int n_eval = 0, n_ign = 0, n_non = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const size_t q = threadIdx.x + (size_t)T * k;  // float4 index within the block
    const float4 dg = reinterpret_cast<const float4*>(gt_d)[gbase4 + q];
    const float4 dt = reinterpret_cast<const float4*>(test_d)[tbase4 + q];
    bool og[4], ot[4];
    eval_load_observed<TSDF>(gt_o, gbase4 + q, og);
    eval_load_observed<TSDF>(test_o, tbase4 + q, ot);
    const float vg[4] = {dg.x, dg.y, dg.z, dg.w}, vt[4] = {dt.x, dt.y, dt.z, dt.w};
    float e4[4];
    uint32_t set4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      e4[j] = 0.0f;
      if (!og[j] || !ot[j]) {
        ++n_non;
      } else if ((ign_test && vt[j] < 0.0f) || (ign_gt && vg[j] < 0.0f)) {
        ++n_ign;
      } else {
        const float e = vt[j] - vg[j];
        const float ae = fabsf(e);
        e4[j] = e;
        set4 |= 1u << (8 * j);
        sum += (double)(e * e);
        mx = fmaxf(mx, ae);
        mn = fminf(mn, ae);
        ++n_eval;
      }
    }
    if (err_d) reinterpret_cast<float4*>(err_d)[ebase4 + q] = make_float4(e4[0], e4[1], e4[2], e4[3]);
    if (err_set) reinterpret_cast<uint32_t*>(err_set)[ebase4 + q] = set4;
  }
  if (err_bi && threadIdx.x < 3) err_bi[3 * (size_t)err_pos[t] + threadIdx.x] = test_bi[3 * (size_t)t + threadIdx.x];
  eval_wave_fold(sum, mx, mn, n_eval, n_ign, n_non);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    s_sum[w] = sum;
    s_max[w] = mx;
    s_min[w] = mn;
    s_cnt[w][0] = n_eval;
    s_cnt[w][1] = n_ign;
    s_cnt[w][2] = n_non;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    EvalPartial p{s_sum[0], s_max[0], s_min[0], s_cnt[0][0], s_cnt[0][1], s_cnt[0][2], 0};
#pragma unroll
    for (int i = 1; i < W; ++i) {  // the waves in order
      p.sum += s_sum[i];
      p.max_abs = fmaxf(p.max_abs, s_max[i]);
      p.min_abs = fminf(p.min_abs, s_min[i]);
      p.n_eval += s_cnt[i][0];
      p.n_ign += s_cnt[i][1];
      p.n_non += s_cnt[i][2];
    }
    part[t] = p;
  }
}

// One workgroup of 1024 threads: partial b to thread b mod 1024 in ascending b, the wave tree, the waves in order; the gt
// blocks without a test block (probed in the test submap's block table) add vps^3 non-overlapping voxels each.
__global__ __launch_bounds__(1024) void eval_fold_kernel(const EvalPartial* __restrict__ part, int n_test,
                                                         const int32_t* __restrict__ has, const int32_t* __restrict__ gt_bi,
                                                         int n_gt, EvalLut test, int vox, EvalTotals* __restrict__ out) {
  constexpr int W = 16;
  __shared__ double s_sum[W];
  __shared__ float s_max[W], s_min[W];
  __shared__ long long s_cnt[W][4];
  double sum = 0.0;
  float mx = 0.0f, mn = INFINITY;
  long long n_eval = 0, n_ign = 0, n_non = 0, n_err = 0;
  for (int b = threadIdx.x; b < n_test; b += 1024) {
    const EvalPartial p = part[b];
    sum += p.sum;
    mx = fmaxf(mx, p.max_abs);
    mn = fminf(mn, p.min_abs);
    n_eval += p.n_eval;
    n_ign += p.n_ign;
    n_non += p.n_non;
    n_err += has[b];
  }
  for (int b = threadIdx.x; b < n_gt; b += 1024)
    if (eval_lut_find(test, gt_bi + 3 * (size_t)b) < 0) n_non += vox;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_down(sum, o);
    mx = fmaxf(mx, __shfl_down(mx, o));
    mn = fminf(mn, __shfl_down(mn, o));
    n_eval += __shfl_down(n_eval, o);
    n_ign += __shfl_down(n_ign, o);
    n_non += __shfl_down(n_non, o);
    n_err += __shfl_down(n_err, o);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    s_sum[w] = sum;
    s_max[w] = mx;
    s_min[w] = mn;
    s_cnt[w][0] = n_eval;
    s_cnt[w][1] = n_ign;
    s_cnt[w][2] = n_non;
    s_cnt[w][3] = n_err;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    EvalTotals r{s_sum[0], s_max[0], s_min[0], s_cnt[0][0], s_cnt[0][1], s_cnt[0][2], s_cnt[0][3]};
    for (int i = 1; i < W; ++i) {
      r.sum += s_sum[i];
      r.max_abs = fmaxf(r.max_abs, s_max[i]);
      r.min_abs = fminf(r.min_abs, s_min[i]);
      r.n_eval += s_cnt[i][0];
      r.n_ign += s_cnt[i][1];
      r.n_non += s_cnt[i][2];
      r.n_err_blocks += s_cnt[i][3];
    }
    *out = r;
  }
}

}  // namespace vgx

using namespace vgx;

namespace {

EvalLut lut_of(vgx_submap sm) {
  return EvalLut{sm->d_lut, make_int3(sm->lut_min[0], sm->lut_min[1], sm->lut_min[2]),
                 make_int3(sm->lut_dim[0], sm->lut_dim[1], sm->lut_dim[2])};
}

bool layer_resident(vgx_submap sm, int32_t layer) {
  if (sm->n_blocks == 0) return true;
  return layer == VGX_EVAL_LAYER_ESDF ? (sm->d_esdf_distance && sm->d_esdf_observed) : (sm->d_tsdf_distance && sm->d_tsdf_weight);
}

}  // namespace

namespace vgx {

int eval_check(const char* fn, vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode, const void* details) {
  if (!gt || !test) return VGX_ERR_INVALID;
  vgx_ctx ctx = gt->ctx;
  auto fail = [ctx, fn](const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": " + msg); };
  if (test->ctx != ctx) return fail("the submaps belong to different contexts");
  if (!details) return fail("NULL details");
  if (layer != VGX_EVAL_LAYER_ESDF && layer != VGX_EVAL_LAYER_TSDF) return fail("layer is neither ESDF nor TSDF");
  if (mode < VGX_EVAL_ALL_VOXELS || mode > VGX_EVAL_IGNORE_BEHIND_ALL) return fail("mode out of range");
  if (gt->voxel_size != test->voxel_size || gt->vps != test->vps)
    return fail("voxel_size / voxels_per_side differ (CHECK_EQ in the reference)");
  if (!layer_resident(gt, layer) || !layer_resident(test, layer))
    return fail(std::string(layer == VGX_EVAL_LAYER_ESDF ? "ESDF" : "TSDF") + " layer not resident (released, or never generated)");
  return VGX_OK;
}

int eval_enqueue(vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode, bool want_index, bool want_distance, bool want_set,
                 EvalDevice& D) {
  vgx_ctx ctx = gt->ctx;
  hipStream_t st = ctx->stream;
  const int vps = test->vps, vox = vps * vps * vps;
  const int n_test = test->n_blocks, n_gt = gt->n_blocks;
  const bool tsdf = layer == VGX_EVAL_LAYER_TSDF;
  const bool want_err = want_index || want_distance || want_set;
  VGX_HIP(ctx, D.tot.alloc(sizeof(EvalTotals)));
  if (n_test > 0) {
    VGX_HIP(ctx, D.slot.alloc((size_t)n_test * 4));
    VGX_HIP(ctx, D.has.alloc((size_t)n_test * 4));
    VGX_HIP(ctx, D.part.alloc((size_t)n_test * sizeof(EvalPartial)));
    hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)((n_test + 255) / 256)), dim3(256), 0, st, test->d_block_index, n_test,
                       lut_of(gt), D.slot.as<int32_t>(), D.has.as<int32_t>());
    VGX_HIP(ctx, hipGetLastError());
    if (want_err) {
      VGX_HIP(ctx, D.pos.alloc((size_t)n_test * 4));
      auto scan = [&](void* tmp, size_t& bytes) {
        return rocprim::exclusive_scan(tmp, bytes, D.has.as<int32_t>(), D.pos.as<int32_t>(), 0, (size_t)n_test, rocprim::plus<int32_t>(),
                                       st);
      };
      VGX_HIP(ctx, run_with_temp(D.tmp, scan));
      // room for every test block: the error blocks are the test blocks with a gt counterpart
      if (want_distance) VGX_HIP(ctx, D.ed.alloc((size_t)n_test * vox * 4));
      if (want_set) VGX_HIP(ctx, D.es.alloc((size_t)n_test * vox));
      if (want_index) VGX_HIP(ctx, D.ebi.alloc((size_t)n_test * 12));
    }
    const float* gd = tsdf ? gt->d_tsdf_distance : gt->d_esdf_distance;
    const void* go = tsdf ? (const void*)gt->d_tsdf_weight : (const void*)gt->d_esdf_observed;
    const float* td = tsdf ? test->d_tsdf_distance : test->d_esdf_distance;
    const void* to = tsdf ? (const void*)test->d_tsdf_weight : (const void*)test->d_esdf_observed;
    auto kernel = vps == 16 ? (tsdf ? eval_block_kernel<16, true> : eval_block_kernel<16, false>)
                            : (tsdf ? eval_block_kernel<8, true> : eval_block_kernel<8, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n_test), dim3(vps == 16 ? 256 : 128), 0, st, D.slot.as<int32_t>(), gd, go, td, to,
                       test->d_block_index, (int)mode, D.part.as<EvalPartial>(), want_err ? D.pos.as<int32_t>() : nullptr,
                       D.ed.as<float>(), D.es.as<uint8_t>(), D.ebi.as<int32_t>());
    VGX_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(1024), 0, st, D.part.as<EvalPartial>(), n_test, D.has.as<int32_t>(),
                     gt->d_block_index, n_gt, lut_of(test), vox, D.tot.as<EvalTotals>());
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

void eval_details(const EvalTotals& tot, vgx_voxel_evaluation_details* details) {
  vgx_voxel_evaluation_details r{};
  r.total_squared_error = tot.sum;
  r.num_evaluated_voxels = tot.n_eval;
  r.num_ignored_voxels = tot.n_ign;
  r.num_overlapping_voxels = tot.n_eval + tot.n_ign;
  r.num_non_overlapping_voxels = tot.n_non;
  r.rmse = tot.n_eval > 0 ? (float)std::sqrt(tot.sum / (double)tot.n_eval) : 0.0f;
  r.max_error = tot.max_abs;
  r.min_error = 0.0f;  // voxblox: initialised to 0, then only min() [recalled]
  r.min_abs_error = tot.n_eval > 0 ? tot.min_abs : 0.0f;
  *details = r;
}

}  // namespace vgx

extern "C" int vgx_evaluate_layers_rmse(vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode,
                                        vgx_voxel_evaluation_details* details, int32_t* error_block_index,
                                        float* error_distance, uint8_t* error_set, int32_t* n_error_blocks) {
  int rc = eval_check("vgx_evaluate_layers_rmse", gt, test, layer, mode, details);
  if (rc != VGX_OK) return rc;
  vgx_ctx ctx = gt->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int vox = test->vps * test->vps * test->vps;
  EvalDevice D;
  rc = eval_enqueue(gt, test, layer, mode, error_block_index != nullptr, error_distance != nullptr, error_set != nullptr, D);
  if (rc != VGX_OK) return rc;
  EvalTotals tot{};
  VGX_HIP(ctx, hipMemcpyAsync(&tot, D.tot.p, sizeof(tot), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  const size_t m = (size_t)tot.n_err_blocks;
  if (m > 0) {
    if (error_distance) VGX_HIP(ctx, hipMemcpyAsync(error_distance, D.ed.p, m * vox * 4, hipMemcpyDeviceToHost, st));
    if (error_set) VGX_HIP(ctx, hipMemcpyAsync(error_set, D.es.p, m * vox, hipMemcpyDeviceToHost, st));
    if (error_block_index) VGX_HIP(ctx, hipMemcpyAsync(error_block_index, D.ebi.p, m * 12, hipMemcpyDeviceToHost, st));
    VGX_HIP(ctx, hipStreamSynchronize(st));
  }
  eval_details(tot, details);
  if (n_error_blocks) *n_error_blocks = (int32_t)tot.n_err_blocks;
  return VGX_OK;
}
