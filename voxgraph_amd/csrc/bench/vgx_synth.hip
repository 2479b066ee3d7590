// Benchmark tooling: the analytic "city" scene of oracle/synth.py, generated on
// the device so that BASELINE config 3 (200 submaps @ 256^3 = 3.4 G voxels) is
// practical.  Bit-for-bit mirror of synth.city_sdf / synth.make_submap (checked
// in tests/test_synth_scene.py).  Not part of the reference's interface.
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "vgx_internal.h"
#include "voxgraph_amd_bench.h"

#pragma clang fp contract(off)

namespace vgx {

__device__ __forceinline__ uint32_t fmix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ float city_uniform(int ci, int cj, uint32_t seed, uint32_t k) {
  uint32_t h = ((uint32_t)ci * 73856093u) ^ ((uint32_t)cj * 19349663u) ^ (seed * 83492791u);
  h = fmix(h + k * 0x9E3779B9u);
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

__device__ float city_sdf(float x, float y, float z, uint32_t seed) {
  const float CELL = 25.6f;
  int ci0 = (int)floorf(x / CELL), cj0 = (int)floorf(y / CELL);
  float d = z;
  for (int di = -1; di <= 1; ++di)
    for (int dj = -1; dj <= 1; ++dj) {
      int ci = ci0 + di, cj = cj0 + dj;
      float u0 = city_uniform(ci, cj, seed, 0), u1 = city_uniform(ci, cj, seed, 1);
      float u2 = city_uniform(ci, cj, seed, 2), u3 = city_uniform(ci, cj, seed, 3);
      float u4 = city_uniform(ci, cj, seed, 4);
      float cx = ((float)ci + 0.5f) * CELL + (u0 - 0.5f) * 6.0f;
      float cy = ((float)cj + 0.5f) * CELL + (u1 - 0.5f) * 6.0f;
      float hx = 4.0f + 5.0f * u2, hy = 4.0f + 5.0f * u3;
      float top = 6.0f + 24.0f * u4;
      float cz = (top - 10.0f) * 0.5f, hz = (top + 10.0f) * 0.5f;
      float qx = fabsf(x - cx) - hx, qy = fabsf(y - cy) - hy, qz = fabsf(z - cz) - hz;
      float ox = fmaxf(qx, 0.0f), oy = fmaxf(qy, 0.0f), oz = fmaxf(qz, 0.0f);
      float outside = sqrtf(ox * ox + oy * oy + oz * oz);
      float inside = fminf(fmaxf(qx, fmaxf(qy, qz)), 0.0f);
      d = fminf(d, outside + inside);
    }
  return d;
}

template <int VPS>
__global__ __launch_bounds__(256) void synth_city_kernel(
    const int32_t* __restrict__ block_index, float voxel_size, float block_size, float cos_yaw,
    float sin_yaw, float tx, float ty, float tz, float trunc, float two_trunc, float esdf_max,
    float weight, uint32_t seed, float* __restrict__ tsdf_d, float* __restrict__ tsdf_w,
    float* __restrict__ esdf_d, uint8_t* __restrict__ esdf_obs) {
  constexpr int VOX = VPS * VPS * VPS;
  const int b = blockIdx.x;
  const float ox = (float)block_index[3 * b + 0] * block_size;
  const float oy = (float)block_index[3 * b + 1] * block_size;
  const float oz = (float)block_index[3 * b + 2] * block_size;
  for (int v = threadIdx.x; v < VOX; v += 256) {
    int ix = v % VPS, iy = (v / VPS) % VPS, iz = v / (VPS * VPS);
    float px = ox + ((float)ix + 0.5f) * voxel_size;
    float py = oy + ((float)iy + 0.5f) * voxel_size;
    float pz = oz + ((float)iz + 0.5f) * voxel_size;
    float wx = (cos_yaw * px - sin_yaw * py) + tx;
    float wy = (sin_yaw * px + cos_yaw * py) + ty;
    float wz = pz + tz;
    float d = city_sdf(wx, wy, wz, seed);
    size_t at = (size_t)b * VOX + v;
    tsdf_d[at] = fminf(fmaxf(d, -trunc), trunc);
    tsdf_w[at] = fabsf(d) <= two_trunc ? weight : 0.0f;
    esdf_d[at] = fminf(fmaxf(d, -esdf_max), esdf_max);
    esdf_obs[at] = fabsf(d) <= esdf_max ? 1 : 0;
  }
}

// One thread per LiDAR ray: sphere tracing of city_sdf (a distance bound, exact outside
// the buildings), then a few bisection steps on the sign change for a crisp surface point.
__global__ __launch_bounds__(256) void synth_city_scan_kernel(float sx, float sy, float sz,
                                                              float cos_yaw, float sin_yaw, int n_az,
                                                              int n_el, float el_span, float max_range,
                                                              uint32_t seed, float* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_az * n_el) return;
  int ia = i % n_az, ie = i / n_az;
  float az = -3.14159265f + 6.2831853f * ((float)ia + 0.5f) / (float)n_az;
  float el = n_el > 1 ? -0.5f * el_span + el_span * (float)ie / (float)(n_el - 1) : 0.0f;
  float dx = cosf(el) * cosf(az), dy = cosf(el) * sinf(az), dz = sinf(el);   // sensor frame
  float wx = cos_yaw * dx - sin_yaw * dy, wy = sin_yaw * dx + cos_yaw * dy, wz = dz;
  float t = 0.2f, hit = 2.0f * max_range;
  for (int it = 0; it < 256 && t < max_range; ++it) {
    float d = city_sdf(sx + t * wx, sy + t * wy, sz + t * wz, seed);
    if (d < 1e-3f) {
      float lo = fmaxf(t - 0.05f, 0.0f), hi = t;
      for (int b = 0; b < 12; ++b) {
        float mid = 0.5f * (lo + hi);
        if (city_sdf(sx + mid * wx, sy + mid * wy, sz + mid * wz, seed) > 0.0f) lo = mid; else hi = mid;
      }
      hit = 0.5f * (lo + hi);
      break;
    }
    t += fmaxf(d, 0.01f);
  }
  out[3 * i] = dx * hit;
  out[3 * i + 1] = dy * hit;
  out[3 * i + 2] = dz * hit;
}

// vgx_bench_atomic_roundtrip: every lane runs `chain` DEPENDENT device-scope exchanges on pseudo-random words of
// a table the size of an approximate hash set -- the memory operation a ray of tsdf_integrate_kernel
// issues once per voxel step and has to wait for before it knows whether to go on.
__global__ __launch_bounds__(256) void atomic_chain_kernel(unsigned long long* __restrict__ table, unsigned mask,
                                                          int chain, unsigned long long* __restrict__ sink) {
  unsigned idx = (blockIdx.x * blockDim.x + threadIdx.x) * 2654435761u + 12345u;
  unsigned long long acc = 0;
  for (int k = 0; k < chain; ++k) {
    const unsigned long long old = atomicExch(&table[idx & mask], (unsigned long long)idx + 1ull);
    acc += old;
    idx = (idx * 1664525u + 1013904223u) ^ (unsigned)(old & 1ull);  // the next address needs this result
  }
  if (acc == 0x123456789abcdefull) *sink = acc;  // keeps the chain alive
}

// vgx_bench_stream_ceiling: what this box's memory system sustains for a launch shaped like the headline kernel --
// `read_bytes` streamed in as float4, `write_bytes` streamed out as non-temporal float4 (the rows are written once and
// never re-read) -- measured in the same process, minutes before the timed region, so that a roofline fraction can be
// read against the box it ran on and not only against the 8 TB/s of the data sheet.  One workgroup walks a contiguous
// slice of both ranges; read_bytes == 0 is a pure fill, write_bytes == read_bytes a float4 copy.
typedef float nt_float4 __attribute__((ext_vector_type(4)));
// ONE float4 position per thread, no loop, a grid of n / 256 workgroups: the shape that reaches the guide's 6.29 TB/s on
// this part (profiles/probes/copy_probe.hip, round 5: copy 6.23-6.37 TB/s, fill 6.8 TB/s, against 4.8-5.3 TB/s for
// grid-stride loops of 2048 to 65536 workgroups with 1 to 8 float4 in flight per thread, and 4.4 TB/s for a private
// contiguous slice per workgroup -- both of which this kernel was, for a day).  Position i reads float4
// floor(i * n_read / N) when that index differs from the one of position i - 1, and likewise writes: the shorter range is
// touched by an evenly spread subset of the lanes, consecutive among themselves.
__global__ __launch_bounds__(256) void stream_ceiling_kernel(const nt_float4* __restrict__ src, unsigned long long read_fp,
                                                            nt_float4* __restrict__ dst, unsigned long long write_fp,
                                                            unsigned long long n_pos) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
  if (i >= n_pos) return;
  // 32.32 fixed point: index of position i in a range of n = fp * N / 2^32 items
  const unsigned long long ri = (i * read_fp) >> 32, rp = i ? ((i - 1ull) * read_fp) >> 32 : ~0ull;
  const unsigned long long wi = (i * write_fp) >> 32, wp = i ? ((i - 1ull) * write_fp) >> 32 : ~0ull;
  const bool rd = read_fp != 0ull && ri != rp, wr = write_fp != 0ull && wi != wp;
  nt_float4 v = {0.0f, 0.0f, 0.0f, (float)threadIdx.x};
  if (rd) v = src[ri];
  if (wr) __builtin_nontemporal_store(v, &dst[wi]);
  else if (rd && v.x == 1.2345e30f) dst[0] = v;  // keeps a read-only position's load alive
}

}  // namespace vgx

using namespace vgx;

extern "C" int vgx_bench_atomic_roundtrip(vgx_ctx ctx, int64_t table_bytes, int32_t waves, int32_t chain,
                                          float* ns_per_step) {
  if (!ctx || !ns_per_step || table_bytes < 8 || (table_bytes & (table_bytes - 1)) || waves <= 0 || chain <= 0)
    return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  DeviceBuffer s_table;
  VGX_HIP(ctx, s_table.alloc((size_t)table_bytes + 8));
  unsigned long long* table = s_table.as<unsigned long long>();
  hipEvent_t e[3];
  for (auto& ev : e) (void)hipEventCreate(&ev);
  int rc = VGX_OK;
  const unsigned mask = (unsigned)(table_bytes / 8 - 1);
  const dim3 grid((unsigned)((waves * 64 + 255) / 256)), block(waves * 64 < 256 ? waves * 64 : 256);
  unsigned long long* sink = table + table_bytes / 8;
  float ms1 = 0.0f, ms2 = 0.0f;
  if (hipMemsetAsync(table, 0, (size_t)table_bytes + 8, ctx->stream) != hipSuccess) rc = VGX_ERR_HIP;
  if (rc == VGX_OK) {
    hipLaunchKernelGGL(atomic_chain_kernel, grid, block, 0, ctx->stream, table, mask, chain, sink);  // warm
    (void)hipEventRecord(e[0], ctx->stream);
    hipLaunchKernelGGL(atomic_chain_kernel, grid, block, 0, ctx->stream, table, mask, chain, sink);
    (void)hipEventRecord(e[1], ctx->stream);
    hipLaunchKernelGGL(atomic_chain_kernel, grid, block, 0, ctx->stream, table, mask, 3 * chain, sink);
    (void)hipEventRecord(e[2], ctx->stream);
    if (hipEventSynchronize(e[2]) != hipSuccess || hipEventElapsedTime(&ms1, e[0], e[1]) != hipSuccess ||
        hipEventElapsedTime(&ms2, e[1], e[2]) != hipSuccess)
      rc = VGX_ERR_HIP;
  }
  for (auto& ev : e) (void)hipEventDestroy(ev);
  if (rc != VGX_OK) return set_error(ctx, rc, "vgx_bench_atomic_roundtrip: HIP failure");
  // two launches of `chain` and 3 x `chain` steps: the difference cancels the launch itself
  *ns_per_step = (ms2 - ms1) * 1e6f / (2.0f * (float)chain);
  return VGX_OK;
}

extern "C" int vgx_bench_stream_ceiling(vgx_ctx ctx, const void* d_src, int64_t read_bytes, void* d_dst,
                                        int64_t write_bytes, int32_t launches, float* ms_per_launch) {
  if (!ctx || !ms_per_launch || read_bytes < 0 || write_bytes < 0 || ((read_bytes | write_bytes) & 15) || launches <= 0 ||
      (read_bytes > 0 && !d_src) || (write_bytes > 0 && !d_dst) || read_bytes + write_bytes == 0)
    return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipEvent_t e[2];
  for (auto& ev : e) (void)hipEventCreate(&ev);
  int rc = VGX_OK;
  float ms = 0.0f;
  const unsigned long long nr = (unsigned long long)read_bytes / 16, nw = (unsigned long long)write_bytes / 16;
  const unsigned long long n_pos = nr > nw ? nr : nw;
  // fp = ceil(n * 2^32 / N) capped at 2^32: position N - 1 maps to item n - 1 at most
  auto ratio = [&](unsigned long long nn) -> unsigned long long {
    if (nn == 0) return 0ull;
    if (nn == n_pos) return 1ull << 32;
    return (unsigned long long)(((unsigned __int128)nn << 32) / n_pos);
  };
  const unsigned long long rf = ratio(nr), wf = ratio(nw);
  const dim3 grid((unsigned)((n_pos + 255ull) / 256ull)), block(256);
  hipLaunchKernelGGL(stream_ceiling_kernel, grid, block, 0, ctx->stream, (const nt_float4*)d_src, rf, (nt_float4*)d_dst, wf,
                     n_pos);  // warm
  (void)hipEventRecord(e[0], ctx->stream);
  for (int k = 0; k < launches; ++k)
    hipLaunchKernelGGL(stream_ceiling_kernel, grid, block, 0, ctx->stream, (const nt_float4*)d_src, rf, (nt_float4*)d_dst, wf,
                       n_pos);
  (void)hipEventRecord(e[1], ctx->stream);
  if (hipGetLastError() != hipSuccess || hipEventSynchronize(e[1]) != hipSuccess ||
      hipEventElapsedTime(&ms, e[0], e[1]) != hipSuccess)
    rc = VGX_ERR_HIP;
  for (auto& ev : e) (void)hipEventDestroy(ev);
  if (rc != VGX_OK) return set_error(ctx, rc, "vgx_bench_stream_ceiling: HIP failure");
  *ms_per_launch = ms / (float)launches;
  return VGX_OK;
}

extern "C" int vgx_synth_city_scan(vgx_ctx ctx, const double pose[4], int32_t n_az, int32_t n_el,
                                   float el_span, float max_range, uint32_t seed, void* d_points) {
  if (!ctx || !pose || !d_points || n_az <= 0 || n_el <= 0) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const int n = n_az * n_el;
  hipLaunchKernelGGL(synth_city_scan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->tsdf_stream,
                     (float)pose[0], (float)pose[1], (float)pose[2], (float)std::cos(pose[3]),
                     (float)std::sin(pose[3]), n_az, n_el, el_span, max_range, seed, (float*)d_points);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

extern "C" int vgx_synth_city_submap(vgx_ctx ctx, int32_t submap_id, float voxel_size, int32_t vps,
                                     const int32_t block_min[3], const int32_t block_dims[3],
                                     float truncation, float esdf_max, float tsdf_weight,
                                     const double true_pose[4], uint32_t seed,
                                     int32_t build_tsdf_grid, vgx_submap* out) {
  if (!ctx || !out || !block_min || !block_dims || !true_pose) return VGX_ERR_INVALID;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (vps != 16 && vps != 8)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_synth_city_submap: voxels_per_side must be 8 or 16");
  int64_t nb64 = (int64_t)block_dims[0] * block_dims[1] * block_dims[2];
  if (!(voxel_size > 0) || block_dims[0] <= 0 || block_dims[1] <= 0 || block_dims[2] <= 0 || nb64 > (1 << 24))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_synth_city_submap: bad geometry");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  vgx_submap sm = new (std::nothrow) vgx_submap_s();
  if (!sm) return set_error(ctx, VGX_ERR_NOMEM, "vgx_synth_city_submap: out of host memory");
  const int nb = (int)nb64;
  sm->ctx = ctx;
  sm->id = submap_id;
  sm->vps = vps;
  sm->n_blocks = nb;
  sm->voxel_size = voxel_size;
  sm->voxel_size_inv = 1.0f / voxel_size;
  sm->block_size = (float)vps * voxel_size;
  sm->block_size_inv = 1.0f / sm->block_size;
  // same block order as synth.dense_block_index: x slowest, z fastest
  sm->block_index.resize(3 * (size_t)nb);
  size_t k = 0;
  for (int x = 0; x < block_dims[0]; ++x)
    for (int y = 0; y < block_dims[1]; ++y)
      for (int z = 0; z < block_dims[2]; ++z) {
        sm->block_index[k++] = block_min[0] + x;
        sm->block_index[k++] = block_min[1] + y;
        sm->block_index[k++] = block_min[2] + z;
      }
  int rc = build_block_lut(sm);
  const size_t nvox = (size_t)nb * vps * vps * vps;
  if (rc == VGX_OK) {
    if (sm->d_block_index.alloc_n(3 * (size_t)nb) != hipSuccess || sm->d_tsdf_distance.alloc_n(nvox) != hipSuccess ||
        sm->d_tsdf_weight.alloc_n(nvox) != hipSuccess || sm->d_esdf_distance.alloc_n(nvox) != hipSuccess ||
        sm->d_esdf_observed.alloc_n(nvox) != hipSuccess)
      rc = set_error(ctx, VGX_ERR_NOMEM, "vgx_synth_city_submap: device allocation failed");
  }
  if (rc == VGX_OK &&
      hipMemcpy(sm->d_block_index, sm->block_index.data(), 3 * (size_t)nb * sizeof(int32_t),
                hipMemcpyHostToDevice) != hipSuccess)
    rc = set_error(ctx, VGX_ERR_HIP, "vgx_synth_city_submap: block index upload failed");
  if (rc == VGX_OK) {
    // synth.pose_apply: F(cos(yaw)), F(sin(yaw)) from double trig
    float c = (float)std::cos(true_pose[3]), s = (float)std::sin(true_pose[3]);
    float two_trunc = 2.0f * truncation;
    if (vps == 16)
      hipLaunchKernelGGL(synth_city_kernel<16>, dim3(nb), dim3(256), 0, ctx->stream,
                         sm->d_block_index, sm->voxel_size, sm->block_size, c, s,
                         (float)true_pose[0], (float)true_pose[1], (float)true_pose[2], truncation,
                         two_trunc, esdf_max, tsdf_weight, seed, sm->d_tsdf_distance,
                         sm->d_tsdf_weight, sm->d_esdf_distance, sm->d_esdf_observed);
    else
      hipLaunchKernelGGL(synth_city_kernel<8>, dim3(nb), dim3(256), 0, ctx->stream,
                         sm->d_block_index, sm->voxel_size, sm->block_size, c, s,
                         (float)true_pose[0], (float)true_pose[1], (float)true_pose[2], truncation,
                         two_trunc, esdf_max, tsdf_weight, seed, sm->d_tsdf_distance,
                         sm->d_tsdf_weight, sm->d_esdf_distance, sm->d_esdf_observed);
    if (hipGetLastError() != hipSuccess) rc = set_error(ctx, VGX_ERR_HIP, "vgx_synth_city_submap: launch failed");
  }
  if (rc == VGX_OK && build_tsdf_grid) rc = launch_brickify(sm, 0);
  if (rc == VGX_OK) rc = launch_brickify(sm, 1);
  if (rc != VGX_OK) {
    vgx_submap_destroy(sm);
    return rc;
  }
  *out = sm;
  return VGX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// vgx_bench_alloc_scattered: device memory whose PHYSICAL pages are deliberately out of order.  The materialising pass runs
// at 4.4 ms on arrays whose pages happen to lie scattered, at 5.4 ms on others and at 7.1 ms on arrays that are one physical
// run (profiles/r05_points_placement.txt); this allocator makes the scattered case on purpose: an address range reserved
// through the virtual-memory API, one physical allocation per `chunk_bytes`, mapped in a shuffled order (seed 0: in order).
namespace {
struct ScatteredRange {
  size_t bytes = 0;
  std::vector<hipMemGenericAllocationHandle_t> handles;
};
std::mutex g_scattered_mu;
std::map<void*, ScatteredRange> g_scattered;
}  // namespace

extern "C" int vgx_bench_alloc_scattered(vgx_ctx ctx, int64_t bytes, int64_t chunk_bytes, uint32_t seed, void** out) {
  if (!ctx || !out || bytes <= 0 || chunk_bytes <= 0) return VGX_ERR_INVALID;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = ctx->device;
  size_t gran = 0;
  VGX_HIP(ctx, hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
  if (gran == 0) gran = 2u << 20;
  const size_t chunk = ((size_t)chunk_bytes + gran - 1) / gran * gran;
  const size_t n = ((size_t)bytes + chunk - 1) / chunk;
  const size_t total = n * chunk;
  void* base = nullptr;
  VGX_HIP(ctx, hipMemAddressReserve(&base, total, gran, nullptr, 0));
  ScatteredRange range;
  range.bytes = total;
  int rc = VGX_OK;
  for (size_t i = 0; i < n && rc == VGX_OK; ++i) {
    hipMemGenericAllocationHandle_t h;
    if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) rc = VGX_ERR_NOMEM;
    else range.handles.push_back(h);
  }
  std::vector<size_t> perm(n);
  for (size_t i = 0; i < n; ++i) perm[i] = i;
  if (seed != 0u) {  // Fisher-Yates on a 64-bit LCG
    unsigned long long state = 0x9E3779B97F4A7C15ull ^ ((unsigned long long)seed * 0xD1B54A32D192ED03ull);
    for (size_t i = n; i > 1; --i) {
      state = state * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(perm[i - 1], perm[(size_t)((state >> 33) % i)]);
    }
  }
  size_t mapped = 0;
  for (size_t i = 0; i < n && rc == VGX_OK; ++i) {
    if (hipMemMap((char*)base + i * chunk, chunk, 0, range.handles[perm[i]], 0) != hipSuccess) rc = VGX_ERR_HIP;
    else mapped = i + 1;
  }
  if (rc == VGX_OK) {
    hipMemAccessDesc desc = {};
    desc.location = prop.location;
    desc.flags = hipMemAccessFlagsProtReadWrite;
    if (hipMemSetAccess(base, total, &desc, 1) != hipSuccess) rc = VGX_ERR_HIP;
  }
  if (rc != VGX_OK) {
    (void)hipGetLastError();
    if (mapped) (void)hipMemUnmap(base, mapped * chunk);
    for (auto h : range.handles) (void)hipMemRelease(h);
    (void)hipMemAddressFree(base, total);
    return set_error(ctx, rc, "vgx_bench_alloc_scattered: the virtual-memory API refused (reserve / create / map / set access)");
  }
  {
    std::lock_guard<std::mutex> g(g_scattered_mu);
    g_scattered[base] = std::move(range);
  }
  *out = base;
  return VGX_OK;
}

extern "C" int vgx_bench_free_scattered(vgx_ctx ctx, void* ptr) {
  if (!ctx || !ptr) return VGX_ERR_INVALID;
  ScatteredRange range;
  {
    std::lock_guard<std::mutex> g(g_scattered_mu);
    auto it = g_scattered.find(ptr);
    if (it == g_scattered.end()) return set_error(ctx, VGX_ERR_INVALID, "vgx_bench_free_scattered: not a scattered range");
    range = std::move(it->second);
    g_scattered.erase(it);
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  VGX_HIP(ctx, hipDeviceSynchronize());
  (void)hipMemUnmap(ptr, range.bytes);
  for (auto h : range.handles) (void)hipMemRelease(h);
  (void)hipMemAddressFree(ptr, range.bytes);
  return VGX_OK;
}
