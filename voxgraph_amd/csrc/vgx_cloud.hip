// Point-cloud views of a layer on the device: voxblox_ros ptcloud_vis.h [recalled] -- createDistancePointcloudFromEsdfLayer /
// ...FromTsdfLayer, createSurfaceDistancePointcloudFromTsdfLayer, createSurfacePointcloudFromTsdfLayer and their ...Slice
// forms, as MapEvaluation publishes them (map_evaluation.cpp:39, :105, :106).  An order-preserving stream compaction of
// the voxels that pass a predicate into {voxel centre, distance[, colour]}; the rules are stated in
// include/voxgraph_amd.h (vgx_cloud), the passes and their measurement in DESIGN.md 16.
//
//   1. cloud_count_kernel: one workgroup per block slot, 4 consecutive voxels per thread per step (16-byte loads); a block
//      the slice plane cannot touch, or a slot beyond the layer's block count, counts 0 without reading a voxel
//   2. rocprim::exclusive_scan of the per-block counts (int64); the total comes back once, to size the output
//   3. cloud_emit_kernel: the same classification; positions inside the workgroup from ballots / popcounts per wave and
//      the waves' counts in LDS, in (step, wave) order -- no atomics: the order is that of the voxels' linear indices
// The three source layouts (SRC) are those of vgx_cloud_src.h, shared with the planar map.
#include <algorithm>
#include <cmath>
#include <string>

#include "vgx_cloud_src.h"
#include "vgx_internal.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

struct CloudRule {
  int32_t kind;
  float surface_distance, min_weight;
  int32_t slice_axis;
  float slice_value;
};

// Bit i: voxel index i of this block on the slice axis passes the slice rule |centre - plane| <= voxel_size / 2 + 1e-6f
// (f32).  From the block index alone: 0 rejects the block before any voxel is read, and the voxels of a kept block test
// their bit -- the same comparison either way, so rejecting changes nothing.  No slice: every row.
template <int VPS>
__device__ __forceinline__ uint32_t cloud_slice_rows(const CloudRule& r, const int32_t* bi, float vs) {
  if (r.slice_axis < 0) return (1u << VPS) - 1u;
  const float origin = (float)bi[r.slice_axis] * ((float)VPS * vs);
  const float reach = 0.5f * vs + 1e-6f;
  uint32_t rows = 0;
#pragma unroll
  for (int i = 0; i < VPS; ++i)
    if (fabsf(voxel_centre(origin, i, vs) - r.slice_value) <= reach) rows |= 1u << i;
  return rows;
}

// The 4 voxels v = 4 q + j of block slot b (x = x0 + j; y and z shared): bit j of the result is set when voxel j is in
// the cloud; d[j] its distance.  Nothing is read when the slice leaves none of the four.
template <int VPS, int SRC>
__device__ __forceinline__ uint32_t cloud_classify4(const CloudSrc& s, const CloudRule& r, uint32_t rows, size_t b, int q,
                                                    float d[4]) {
  constexpr int Q = VPS / 4;  // float4 per voxel row
  const int x0 = 4 * (q % Q), y = (q / Q) % VPS, z = q / (Q * VPS);
  uint32_t in;
  if (r.slice_axis == 1) in = ((rows >> y) & 1u) ? 0xfu : 0u;
  else if (r.slice_axis == 2) in = ((rows >> z) & 1u) ? 0xfu : 0u;
  else in = (rows >> x0) & 0xfu;
  if (in == 0u) return 0u;
  const size_t at4 = b * (size_t)(VPS * VPS * Q) + (size_t)q;
  bool seen[4];
  if (SRC == kCloudSrcPacked) {
    const ulonglong2 a = reinterpret_cast<const ulonglong2*>(s.words)[2 * at4];
    const ulonglong2 c = reinterpret_cast<const ulonglong2*>(s.words)[2 * at4 + 1];
    const unsigned long long w[4] = {a.x, a.y, c.x, c.y};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      d[j] = __uint_as_float((uint32_t)w[j]);
      seen[j] = __uint_as_float((uint32_t)(w[j] >> 32)) > r.min_weight;
    }
  } else {
    const float4 dd = reinterpret_cast<const float4*>(s.dist)[at4];
    d[0] = dd.x;
    d[1] = dd.y;
    d[2] = dd.z;
    d[3] = dd.w;
    if (SRC == kCloudSrcTsdf) {
      const float4 w = reinterpret_cast<const float4*>(s.seen)[at4];
      seen[0] = w.x > r.min_weight;
      seen[1] = w.y > r.min_weight;
      seen[2] = w.z > r.min_weight;
      seen[3] = w.w > r.min_weight;
    } else {
      const uint32_t o = reinterpret_cast<const uint32_t*>(s.seen)[at4];
#pragma unroll
      for (int j = 0; j < 4; ++j) seen[j] = ((o >> (8 * j)) & 0xffu) != 0u;
    }
  }
  uint32_t pass = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (seen[j] && (r.kind == VGX_CLOUD_DISTANCE || fabsf(d[j]) < r.surface_distance)) pass |= 1u << j;
  return pass & in;
}

// One workgroup of T = min(256, VOX / 4) threads per block slot, K = VOX / (4 T) steps: thread t holds the voxels
// 4 (t + T k) + j of step k.
template <int VPS, int SRC>
__global__ __launch_bounds__(VPS == 16 ? 256 : 128) void cloud_count_kernel(CloudSrc s, CloudRule r, int slots,
                                                                           long long* __restrict__ counts) {
  constexpr int VOX = VPS * VPS * VPS;
  constexpr int T = VPS == 16 ? 256 : 128;
  constexpr int K = VOX / (4 * T);
  constexpr int W = T / 64;
  __shared__ int s_cnt[W];
  const int b = blockIdx.x;
  const uint32_t rows = b < cloud_live_blocks(s, slots) ? cloud_slice_rows<VPS>(r, s.block_index + 3 * (size_t)b, s.voxel_size) : 0u;
  if (rows == 0u) {  // (uniform)
    if (threadIdx.x == 0) counts[b] = 0;
    return;
  }
  int c = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float d[4];
    c += __popc(cloud_classify4<VPS, SRC>(s, r, rows, (size_t)b, (int)threadIdx.x + T * k, d));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) n += s_cnt[w];
    counts[b] = n;
  }
}

template <int VPS, int SRC>
__global__ __launch_bounds__(VPS == 16 ? 256 : 128) void cloud_emit_kernel(CloudSrc s, CloudRule r,
                                                                          const long long* __restrict__ offsets,
                                                                          float* __restrict__ xyz, float* __restrict__ intensity,
                                                                          uint32_t* __restrict__ rgba) {
  constexpr int VOX = VPS * VPS * VPS;
  constexpr int T = VPS == 16 ? 256 : 128;
  constexpr int K = VOX / (4 * T);
  constexpr int W = T / 64;
  constexpr int Q = VPS / 4;
  __shared__ int s_cnt[K][W];
  const int b = blockIdx.x;
  const long long first = offsets[b];
  if (offsets[b + 1] == first) return;  // (uniform) no point: a rejected block, a slot beyond the layer, or nothing passed
  const int32_t* bi = s.block_index + 3 * (size_t)b;
  const float vs = s.voxel_size;
  const uint32_t rows = cloud_slice_rows<VPS>(r, bi, vs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  float d[K][4];
  uint32_t pass[K];
  int before[K];  // points of this step in the lanes below this one
#pragma unroll
  for (int k = 0; k < K; ++k) {
    pass[k] = cloud_classify4<VPS, SRC>(s, r, rows, (size_t)b, (int)threadIdx.x + T * k, d[k]);
    int mine = 0, all = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long m = __ballot((pass[k] >> j) & 1u);
      mine += __popcll(m & below);
      all += __popcll(m);
    }
    before[k] = mine;
    if (lane == 0) s_cnt[k][wave] = all;
  }
  __syncthreads();
  const float block_size = (float)VPS * vs;
  const float ox = (float)bi[0] * block_size, oy = (float)bi[1] * block_size, oz = (float)bi[2] * block_size;
  long long base = first;  // of (step k, wave 0)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int lower = 0, step = 0;  // the waves before this one, in order; then the whole step
#pragma unroll
    for (int w = 0; w < W; ++w) {
      if (w < wave) lower += s_cnt[k][w];
      step += s_cnt[k][w];
    }
    if (pass[k] != 0u) {
      const int q = (int)threadIdx.x + T * k;
      const int x0 = 4 * (q % Q), iy = (q / Q) % VPS, iz = q / (Q * VPS);
      const float y = voxel_centre(oy, iy, vs), z = voxel_centre(oz, iz, vs);
      uint4 colour = make_uint4(0u, 0u, 0u, 0u);
      if (SRC == kCloudSrcPacked && rgba) colour = reinterpret_cast<const uint4*>(s.rgba)[(size_t)b * (VOX / 4) + (size_t)q];
      const uint32_t col[4] = {colour.x, colour.y, colour.z, colour.w};
      long long at = base + lower + before[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if ((pass[k] >> j) & 1u) {
          xyz[3 * (size_t)at + 0] = voxel_centre(ox, x0 + j, vs);
          xyz[3 * (size_t)at + 1] = y;
          xyz[3 * (size_t)at + 2] = z;
          intensity[at] = d[k][j];
          if (SRC == kCloudSrcPacked && rgba) rgba[at] = col[j];
          ++at;
        }
      }
    }
    base += step;
  }
}

}  // namespace vgx

using namespace vgx;

struct vgx_cloud_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  int64_t n_points = 0;  // the cloud held now
  bool has_colors = false;
  // output, grown on demand to exactly what a cloud needs (no slack, no floor)
  DeviceBuffer d_xyz;        // float [cap][3]
  DeviceBuffer d_intensity;  // float [cap]
  DeviceBuffer d_rgba;       // u32 [color_cap] bytes r g b a
};

namespace {

int ensure_points(vgx_cloud C, int64_t n, bool colors) {
  if ((size_t)n * 4 > C->d_intensity.bytes) {
    C->d_rgba.release();
    const hipError_t e = alloc_group({{&C->d_xyz, (size_t)n * 12}, {&C->d_intensity, (size_t)n * 4}});
    if (e != hipSuccess) return alloc_error(C->ctx, e, "cloud: allocating points");
  }
  const hipError_t e = colors ? C->d_rgba.reserve((size_t)n * 4) : hipSuccess;
  return e == hipSuccess ? VGX_OK : alloc_error(C->ctx, e, "cloud: allocating colours");
}

// Refusals shared by the three producers, before anything is written; cfg == NULL: the defaults.
int cloud_check(vgx_ctx ctx, const char* fn, const vgx_cloud_config* cfg, vgx_cloud C, bool source_has_colors, CloudRule* rule) {
  auto fail = [ctx, fn](const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": " + msg); };
  if (!C) return fail("NULL cloud");
  if (C->ctx != ctx) return fail("the cloud belongs to another context");
  vgx_cloud_config c;
  vgx_cloud_config_default(&c);
  if (cfg) c = *cfg;
  if (c.kind != VGX_CLOUD_DISTANCE && c.kind != VGX_CLOUD_SURFACE_DISTANCE && c.kind != VGX_CLOUD_SURFACE_COLOR)
    return fail("unknown kind");
  if (!std::isfinite(c.surface_distance)) return fail("surface_distance is not finite");
  if (!std::isfinite(c.min_weight) || c.min_weight < 0.0f) return fail("min_weight is negative or not finite");
  if (c.slice_axis < -1 || c.slice_axis > 2) return fail("slice_axis is not -1, 0, 1 or 2");
  if (!std::isfinite(c.slice_value)) return fail("slice_value is not finite");
  if (c.kind == VGX_CLOUD_SURFACE_COLOR && !source_has_colors) return fail("VGX_CLOUD_SURFACE_COLOR on a source without colours");
  *rule = CloudRule{c.kind, c.surface_distance, c.min_weight, c.slice_axis, c.slice_value};
  return VGX_OK;
}

template <int VPS, int SRC>
void launch_count(hipStream_t st, const CloudSrc& s, const CloudRule& r, int slots, long long* counts) {
  hipLaunchKernelGGL((cloud_count_kernel<VPS, SRC>), dim3((unsigned)slots), dim3(VPS == 16 ? 256 : 128), 0, st, s, r, slots, counts);
}
template <int VPS, int SRC>
void launch_emit(hipStream_t st, const CloudSrc& s, const CloudRule& r, int slots, const long long* offsets, vgx_cloud C,
                 bool colors) {
  hipLaunchKernelGGL((cloud_emit_kernel<VPS, SRC>), dim3((unsigned)slots), dim3(VPS == 16 ? 256 : 128), 0, st, s, r, offsets,
                     C->d_xyz.as<float>(), C->d_intensity.as<float>(), colors ? C->d_rgba.as<uint32_t>() : nullptr);
}

// The three passes over `slots` block slots on stream st (the caller holds the cloud's and the stream's locks).  `extra`
// bytes at d_extra come back with the total, in the first of the two synchronisations (the evaluation's totals).
int cloud_generate(vgx_ctx ctx, hipStream_t st, int src, int vps, const CloudSrc& s, const CloudRule& r, int slots, vgx_cloud C,
                   void* h_extra, const void* d_extra, size_t extra) {
  const bool colors = r.kind == VGX_CLOUD_SURFACE_COLOR;
  C->n_points = 0;
  C->has_colors = colors;
  long long total = 0;
  DeviceBuffer d_counts, d_offsets, d_tmp;
  if (slots > 0) {
    const size_t n = (size_t)slots + 1;  // the last item is 0: its exclusive sum is the total
    VGX_HIP(ctx, d_counts.alloc(n * 8));
    VGX_HIP(ctx, d_offsets.alloc(n * 8));
    VGX_HIP(ctx, hipMemsetAsync(d_counts.as<long long>() + slots, 0, 8, st));
    if (vps == 16) {
      if (src == kCloudSrcEsdf) launch_count<16, kCloudSrcEsdf>(st, s, r, slots, d_counts.as<long long>());
      else if (src == kCloudSrcTsdf) launch_count<16, kCloudSrcTsdf>(st, s, r, slots, d_counts.as<long long>());
      else launch_count<16, kCloudSrcPacked>(st, s, r, slots, d_counts.as<long long>());
    } else {
      if (src == kCloudSrcEsdf) launch_count<8, kCloudSrcEsdf>(st, s, r, slots, d_counts.as<long long>());
      else if (src == kCloudSrcTsdf) launch_count<8, kCloudSrcTsdf>(st, s, r, slots, d_counts.as<long long>());
      else launch_count<8, kCloudSrcPacked>(st, s, r, slots, d_counts.as<long long>());
    }
    VGX_HIP(ctx, hipGetLastError());
    auto scan = [&](void* tmp, size_t& bytes) {
      return rocprim::exclusive_scan(tmp, bytes, d_counts.as<long long>(), d_offsets.as<long long>(), 0ll, n, rocprim::plus<long long>(),
                                     st);
    };
    VGX_HIP(ctx, run_with_temp(d_tmp, scan));
    VGX_HIP(ctx, hipMemcpyAsync(&total, d_offsets.as<long long>() + slots, 8, hipMemcpyDeviceToHost, st));
  }
  if (extra) VGX_HIP(ctx, hipMemcpyAsync(h_extra, d_extra, extra, hipMemcpyDeviceToHost, st));
  if (slots > 0 || extra) VGX_HIP(ctx, hipStreamSynchronize(st));
  if (total == 0) return VGX_OK;
  const int rc = ensure_points(C, total, colors);
  if (rc != VGX_OK) return rc;
  if (vps == 16) {
    if (src == kCloudSrcEsdf) launch_emit<16, kCloudSrcEsdf>(st, s, r, slots, d_offsets.as<long long>(), C, colors);
    else if (src == kCloudSrcTsdf) launch_emit<16, kCloudSrcTsdf>(st, s, r, slots, d_offsets.as<long long>(), C, colors);
    else launch_emit<16, kCloudSrcPacked>(st, s, r, slots, d_offsets.as<long long>(), C, colors);
  } else {
    if (src == kCloudSrcEsdf) launch_emit<8, kCloudSrcEsdf>(st, s, r, slots, d_offsets.as<long long>(), C, colors);
    else if (src == kCloudSrcTsdf) launch_emit<8, kCloudSrcTsdf>(st, s, r, slots, d_offsets.as<long long>(), C, colors);
    else launch_emit<8, kCloudSrcPacked>(st, s, r, slots, d_offsets.as<long long>(), C, colors);
  }
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, hipStreamSynchronize(st));
  C->n_points = total;
  return VGX_OK;
}

}  // namespace

extern "C" {

void vgx_cloud_config_default(vgx_cloud_config* cfg) {
  if (!cfg) return;
  cfg->kind = VGX_CLOUD_DISTANCE;
  cfg->surface_distance = 0.6f;  // what voxgraph passes (map_evaluation.cpp:39)
  cfg->min_weight = 1e-3f;       // ptcloud_vis.h kMinWeight [recalled]
  cfg->slice_axis = -1;
  cfg->slice_value = 0.0f;
}

int vgx_cloud_create(vgx_ctx ctx, vgx_cloud* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_cloud_create: NULL argument");
  vgx_cloud C = new vgx_cloud_s;
  C->ctx = ctx;
  *out = C;
  return VGX_OK;
}

int vgx_cloud_destroy(vgx_cloud C) {
  if (!C) return VGX_ERR_INVALID;
  (void)hipSetDevice(C->ctx->device);
  delete C;
  return VGX_OK;
}

int vgx_cloud_stats(vgx_cloud C, int64_t* n_points, int32_t* has_colors) {
  if (!C) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(C->mu);
  if (n_points) *n_points = C->n_points;
  if (has_colors) *has_colors = C->has_colors ? 1 : 0;
  return VGX_OK;
}

int vgx_cloud_device_pointers(vgx_cloud C, const float** xyz, const float** intensity, const uint8_t** rgba) {
  if (!C) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(C->mu);
  const bool any = C->n_points > 0;
  if (xyz) *xyz = any ? C->d_xyz.as<float>() : nullptr;
  if (intensity) *intensity = any ? C->d_intensity.as<float>() : nullptr;
  if (rgba) *rgba = any && C->has_colors ? C->d_rgba.as<uint8_t>() : nullptr;
  return VGX_OK;
}

int vgx_cloud_download(vgx_cloud C, float* xyz, float* intensity, uint8_t* rgba) {
  if (!C) return VGX_ERR_INVALID;
  vgx_ctx ctx = C->ctx;
  std::lock_guard<std::mutex> lk(C->mu);
  if (rgba && !C->has_colors) return set_error(ctx, VGX_ERR_INVALID, "vgx_cloud_download: the cloud has no colours");
  if (C->n_points == 0) return VGX_OK;
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the cloud was complete when its producer returned, whichever stream made it)
  const size_t n = (size_t)C->n_points;
  if (xyz) VGX_HIP(ctx, hipMemcpyAsync(xyz, C->d_xyz.p, n * 12, hipMemcpyDeviceToHost, st));
  if (intensity) VGX_HIP(ctx, hipMemcpyAsync(intensity, C->d_intensity.p, n * 4, hipMemcpyDeviceToHost, st));
  if (rgba) VGX_HIP(ctx, hipMemcpyAsync(rgba, C->d_rgba.p, n * 4, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  return VGX_OK;
}

int vgx_submap_layer_cloud(vgx_submap sm, int32_t layer, const vgx_cloud_config* cfg, vgx_cloud C) {
  static const char* kFn = "vgx_submap_layer_cloud";
  if (!sm) return set_error(C ? C->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL submap");
  vgx_ctx ctx = sm->ctx;
  CloudRule rule{};
  int rc = cloud_check(ctx, kFn, cfg, C, false, &rule);
  if (rc != VGX_OK) return rc;
  if (layer != VGX_EVAL_LAYER_ESDF && layer != VGX_EVAL_LAYER_TSDF)
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": layer is neither ESDF nor TSDF");
  const bool tsdf = layer == VGX_EVAL_LAYER_TSDF;
  if (sm->n_blocks > 0 && (tsdf ? (!sm->d_tsdf_distance || !sm->d_tsdf_weight) : (!sm->d_esdf_distance || !sm->d_esdf_observed)))
    return set_error(ctx, VGX_ERR_INVALID,
                     std::string(kFn) + (tsdf ? ": TSDF" : ": ESDF") + " layer not resident (released, or never generated)");
  if (sm->vps != 8 && sm->vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + ": voxels_per_side must be 8 or 16");
  std::lock_guard<std::mutex> cloud_lk(C->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  CloudSrc s{};
  s.block_index = sm->d_block_index;
  s.dist = tsdf ? sm->d_tsdf_distance : sm->d_esdf_distance;
  s.seen = tsdf ? (const void*)sm->d_tsdf_weight : (const void*)sm->d_esdf_observed;
  s.voxel_size = sm->voxel_size;
  return cloud_generate(ctx, ctx->stream, tsdf ? kCloudSrcTsdf : kCloudSrcEsdf, sm->vps, s, rule, sm->n_blocks, C, nullptr, nullptr, 0);
}

int vgx_tsdf_layer_cloud(vgx_tsdf_layer L, const vgx_cloud_config* cfg, vgx_cloud C) {
  static const char* kFn = "vgx_tsdf_layer_cloud";
  if (!L) return set_error(C ? C->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL layer");
  vgx_ctx ctx = L->ctx;
  CloudRule rule{};
  int rc = cloud_check(ctx, kFn, cfg, C, true, &rule);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> cloud_lk(C->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const TsdfLayerDev& d = L->dev;
  if (d.vps != 8 && d.vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + ": voxels_per_side must be 8 or 16");
  CloudSrc s{};
  s.block_index = d.block_index;
  // behind the scans and merges queued on the TSDF stream, whose allocation counter only the device knows: one workgroup
  // per slot of the pool, those beyond the counter count 0
  s.live_blocks = d.n_blocks;
  s.live_blocks_is_64 = 0;
  s.words = d.voxels;
  s.rgba = d.rgba;
  s.voxel_size = d.voxel_size;
  return cloud_generate(ctx, ctx->tsdf_stream, kCloudSrcPacked, d.vps, s, rule, d.max_blocks, C, nullptr, nullptr, 0);
}

int vgx_evaluate_layers_rmse_cloud(vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode,
                                   vgx_voxel_evaluation_details* details, const vgx_cloud_config* cfg, vgx_cloud C) {
  static const char* kFn = "vgx_evaluate_layers_rmse_cloud";
  if (!gt || !test) return set_error(C ? C->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL submap");
  vgx_ctx ctx = gt->ctx;
  CloudRule rule{};
  int rc = cloud_check(ctx, kFn, cfg, C, false, &rule);
  if (rc != VGX_OK) return rc;
  rc = eval_check(kFn, gt, test, layer, mode, details);
  if (rc != VGX_OK) return rc;
  if (test->vps != 8 && test->vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + ": voxels_per_side must be 8 or 16");
  std::lock_guard<std::mutex> cloud_lk(C->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  // the passes of vgx_evaluate_layers_rmse with the error layer kept in device scratch (the same kernels: the same
  // details), then the cloud of that layer: an ESDF-style layer, observed = error_set, distance = e
  EvalDevice D;
  rc = eval_enqueue(gt, test, layer, mode, true, true, true, D);
  if (rc != VGX_OK) return rc;
  CloudSrc s{};
  s.block_index = D.ebi.as<int32_t>();
  s.live_blocks = &D.tot.as<EvalTotals>()->n_err_blocks;
  s.live_blocks_is_64 = 1;
  s.dist = D.ed.as<float>();
  s.seen = D.es.p;
  s.voxel_size = test->voxel_size;
  EvalTotals tot{};
  rc = cloud_generate(ctx, ctx->stream, kCloudSrcEsdf, test->vps, s, rule, test->n_blocks, C, &tot, D.tot.p, sizeof(tot));
  if (rc != VGX_OK) return rc;
  eval_details(tot, details);
  return VGX_OK;
}

}  // extern "C"
