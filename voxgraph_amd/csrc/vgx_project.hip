// The projected map on the device: voxblox::mergeLayerAintoLayerB(submap TSDF layer, T_L_S, layer) [recalled] for n
// submaps in array order -- cblox::SubmapCollection::getProjectedMap() is this on an empty layer with the collection's
// submaps in ID order.  The semantics are stated in include/voxgraph_amd.h (vgx_tsdf_layer_merge_submaps); the layout
// and the kernel in DESIGN.md 10.
//
//   1. per submap, once: which blocks hold a voxel of weight > 0 (block_has_data_kernel, cached on the handle)
//   2. candidate pairs (target block, array position): every such block's corners, grown by one voxel, transformed
//      into the layer frame; the target blocks its box covers (project_pairs_kernel, counted then emitted)
//   3. one radix sort of the 64-bit keys {target block in the candidate box, position}: a target's submaps are then
//      consecutive and in array order; segment starts by a flagged select
//   4. one workgroup per target block (project_merge_kernel): the block's voxels in registers, every candidate submap
//      interpolated at every voxel centre and merged if any voxel interpolated; stored (and allocated) only if some
//      submap contributed.  No atomics on voxels: the result does not depend on scheduling.
// voxblox::transformLayer (vgx_tsdf_layer_transform_submap) is the same passes with n = 1 into an empty layer; only step 4
// differs (COPY: the interpolated voxel is stored as it is, not merged).
#include <cmath>
#include <string>
#include <vector>

#include "vgx_internal.h"
#include "vgx_interp.h"
#include "vgx_pose.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

struct alignas(16) ProjectSrc : LayerTable {
  // tsdf_interp's other fields (the submap's raw layer)
  const float* tsdf_d;
  const float* tsdf_w;
  // candidate pairs
  const int32_t* block_index;
  const uint8_t* has_data;
  float q_ls[4], t_ls[3];  // T_L_S {w, x, y, z}, t: source corners into the layer
  float q_sl[4], t_sl[3];  // T_S_L = T_L_S.inverse(): layer voxel centres into the source
  const uint32_t* tsdf_rgba;  // the submap's colours, or null (read by the COLOR instantiations only)
};

// target-block range [lo, hi] of one source block (its box grown by one voxel, 8 corners into the layer frame),
// clipped to the candidate box
__device__ __forceinline__ void target_range(const ProjectSrc& s, const int32_t* bi, int3 box_lo, int3 box_dim, int lo[3],
                                             int hi[3]) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float o = (float)bi[a] * s.block_size;
      c[a] = ((k >> a) & 1) ? (o + s.block_size) + s.voxel_size : o - s.voxel_size;
    }
    float g[3];
    rigid_apply(s.q_ls, s.t_ls, c, g);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], g[a]);
      mx[a] = fmaxf(mx[a], g[a]);
    }
  }
  const int bl[3] = {box_lo.x, box_lo.y, box_lo.z}, bd[3] = {box_dim.x, box_dim.y, box_dim.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = max((int)floorf(mn[a] * s.block_size_inv), bl[a]);
    hi[a] = min((int)floorf(mx[a] * s.block_size_inv), bl[a] + bd[a] - 1);
  }
}

template <int VPS>
__global__ __launch_bounds__(256) void block_has_data_kernel(const float* __restrict__ w, uint8_t* __restrict__ flags) {
  constexpr int VOX = VPS * VPS * VPS;
  const size_t base = (size_t)blockIdx.x * VOX;
  int any = 0;
  for (int i = threadIdx.x; i < VOX; i += 256) any |= w[base + i] > 0.0f;
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flags[blockIdx.x] = any ? 1 : 0;
}

// One thread per source block of any submap (src_first: prefix of the submaps' block counts).  keys == null: count the
// pairs into *cursor; else emit them at positions taken from *cursor (wave-aggregated; the sort fixes the order).
__global__ __launch_bounds__(256) void project_pairs_kernel(const ProjectSrc* __restrict__ src, const int64_t* __restrict__ src_first,
                                                            int n_src, int64_t total, int3 box_lo, int3 box_dim, int pos_bits,
                                                            unsigned long long* __restrict__ keys, unsigned long long* cursor,
                                                            unsigned long long capacity) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
  int s = 0;
  if (g < total) {
    int a = 0, b = n_src;  // last submap with src_first[s] <= g
    while (b - a > 1) {
      const int m = (a + b) >> 1;
      if (src_first[m] <= g) a = m; else b = m;
    }
    s = a;
    const int64_t blk = g - src_first[s];
    if (src[s].has_data[blk]) target_range(src[s], src[s].block_index + 3 * blk, box_lo, box_dim, lo, hi);
  }
  unsigned long long cnt = 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) cnt *= hi[a] >= lo[a] ? (unsigned long long)(hi[a] - lo[a] + 1) : 0ull;
  // wave-inclusive prefix of cnt, one atomic per wave
  const int lane = threadIdx.x & 63;
  unsigned long long inc = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  unsigned long long base = 0;
  if (lane == 63) base = atomicAdd(cursor, inc);
  base = __shfl(base, 63);
  if (!keys || cnt == 0) return;
  unsigned long long at = base + inc - cnt;
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int x = lo[0]; x <= hi[0]; ++x) {
        const unsigned long long cell = (unsigned long long)(x - box_lo.x) +
                                        (unsigned long long)box_dim.x * ((unsigned long long)(y - box_lo.y) +
                                                                         (unsigned long long)box_dim.y * (unsigned long long)(z - box_lo.z));
        if (at < capacity) keys[at] = (cell << pos_bits) | (unsigned long long)s;
        ++at;
      }
}

__global__ __launch_bounds__(256) void segment_heads_kernel(const unsigned long long* __restrict__ keys, uint32_t n, int pos_bits,
                                                            uint8_t* __restrict__ heads) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) heads[i] = (i == 0 || (keys[i] >> pos_bits) != (keys[i - 1] >> pos_bits)) ? 1 : 0;
}

// One workgroup per target block: its existing voxels (or the default voxel) in registers, merged with every candidate
// submap in array order.  PER voxels per thread, VPS^3 / PER threads: 4 x 1024 at vps = 16 (16 x 256 kept 253 VGPRs
// live -- the unrolled gathers and divisions of 16 voxels -- one wave per SIMD), 2 x 256 at vps = 8.
// COPY (transformLayer): the layer is empty and each target has one candidate submap; an interpolated voxel is stored as
// {d, w}, every other voxel of a kept block as (0, 0) -- not the merge, whose (d*w + 0*0) / w need not round back to d.
// COLOR (launched only when a submap of the call has colours): the voxels' rgba words ride along -- a coloured submap's
// interpolated colour (tsdf_color_interp, a second pass over the 8 neighbours) is blended in with the pre-merge weights
// wherever the merge updates the voxel; a colourless submap leaves rgba alone.  The colourless instantiations are the
// kernels they were: every colour line is behind `if (COLOR)`.
template <int VPS, int PER, bool COPY, bool COLOR>
__global__ __launch_bounds__(VPS * VPS * VPS / PER) void project_merge_kernel(const unsigned long long* __restrict__ keys,
                                                                              const uint32_t* __restrict__ seg_start, uint32_t n_pairs,
                                                                              const ProjectSrc* __restrict__ src, TsdfLayerDev L,
                                                                              int3 box_lo, int3 box_dim, int pos_bits) {
  constexpr int VOX = VPS * VPS * VPS;
  constexpr int T = VOX / PER;
  __shared__ int s_slot;
  const uint32_t first = seg_start[blockIdx.x];
  const uint32_t last = blockIdx.x + 1 < gridDim.x ? seg_start[blockIdx.x + 1] : n_pairs;
  const unsigned long long cell = keys[first] >> pos_bits;
  const int bx = box_lo.x + (int)(cell % (unsigned long long)box_dim.x);
  const int by = box_lo.y + (int)((cell / (unsigned long long)box_dim.x) % (unsigned long long)box_dim.y);
  const int bz = box_lo.z + (int)(cell / ((unsigned long long)box_dim.x * (unsigned long long)box_dim.y));
  const int rx = bx - L.lut_min[0], ry = by - L.lut_min[1], rz = bz - L.lut_min[2];
  if ((unsigned)rx >= (unsigned)L.lut_dim[0] || (unsigned)ry >= (unsigned)L.lut_dim[1] || (unsigned)rz >= (unsigned)L.lut_dim[2]) {
    if (threadIdx.x == 0) atomicAdd(L.dropped, (unsigned long long)VOX);  // (the host reserved the box: not reached)
    return;
  }
  int slot = L.lut[rx + L.lut_dim[0] * (ry + L.lut_dim[1] * rz)];
  float d[PER], w[PER];
  uint32_t col[COLOR ? PER : 1];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    d[k] = 0.0f;
    w[k] = 0.0f;
    if (COLOR) col[k] = 0u;
    if (slot >= 0) {
      const unsigned long long v = L.voxels[(size_t)slot * VOX + threadIdx.x + T * k];
      d[k] = __uint_as_float((uint32_t)v);
      w[k] = __uint_as_float((uint32_t)(v >> 32));
      if (COLOR && !COPY) col[k] = L.rgba[(size_t)slot * VOX + threadIdx.x + T * k];
    }
  }
  bool col_touched = false;  // COLOR: a coloured submap contributed (uniform across the workgroup)
  const float vs = L.voxel_size, bs = (float)VPS * L.voxel_size;
  const float ox = (float)bx * bs, oy = (float)by * bs, oz = (float)bz * bs;
  const unsigned long long pos_mask = (1ull << pos_bits) - 1ull;
  bool contributed = false;
  int prev = -1;
  for (uint32_t i = first; i < last; ++i) {
    const int pos = (int)(keys[i] & pos_mask);
    if (pos == prev) continue;  // (the same source reached this target from several of its blocks)
    prev = pos;
    const ProjectSrc& s = src[pos];
    float sd[PER], sw[PER];
    uint32_t sc[COLOR ? PER : 1];
    const uint32_t* const src_rgba = COLOR ? s.tsdf_rgba : nullptr;
    unsigned ok = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int lin = threadIdx.x + T * k;
      const int vx = lin % VPS, vy = (lin / VPS) % VPS, vz = lin / (VPS * VPS);
      // Block::computeCoordinatesFromLinearIndex: origin + (idx + 0.5) * voxel_size
      const float c[3] = {voxel_centre(ox, vx, vs), voxel_centre(oy, vy, vs), voxel_centre(oz, vz, vs)};
      float p[3];
      rigid_apply(s.q_sl, s.t_sl, c, p);
      sd[k] = 0.0f;
      sw[k] = 0.0f;
      const bool hit = tsdf_interp<VPS>(s, p, sd[k], sw[k]);
      if (hit) ok |= 1u << k;
      if (COLOR) sc[k] = (hit && src_rgba) ? tsdf_color_interp<VPS>(s, src_rgba, p) : 0u;  // (else the default voxel's colour)
    }
    if (__syncthreads_or(ok != 0)) {
      contributed = true;
      if (COLOR && src_rgba) col_touched = true;
      if (COPY) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
          const bool hit = (ok >> k) & 1u;
          d[k] = hit ? sd[k] : 0.0f;
          w[k] = hit ? sw[k] : 0.0f;
          if (COLOR) col[k] = sc[k];
        }
        continue;
      }
      // mergeVoxelAIntoVoxelB(A = the interpolated voxel or the default one, B = the layer's)
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const bool hit = (ok >> k) & 1u;
        const float da = hit ? sd[k] : 0.0f, wa = hit ? sw[k] : 0.0f;
        const float wn = wa + w[k];
        if (wn > 0.0f) {
          if (COLOR && src_rgba) col[k] = blended_color(col[k], sc[k], w[k], wa);  // (the pre-merge weights)
          d[k] = (da * wa + d[k] * w[k]) / wn;
          w[k] = wn;
        }
      }
    }
  }
  if (!contributed) return;  // (uniform: every thread saw the same __syncthreads_or)
  if (slot < 0) {
    if (threadIdx.x == 0) {
      s_slot = get_or_allocate_block(L, bx, by, bz);
      if (s_slot < 0) atomicAdd(L.dropped, (unsigned long long)VOX);  // (the host reserved the pool: not reached)
    }
    __syncthreads();
    slot = s_slot;
    if (slot < 0) return;
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) L.voxels[(size_t)slot * VOX + threadIdx.x + T * k] = pack_voxel(d[k], w[k]);
  if (COLOR && col_touched) {  // (a block only colourless submaps reached keeps its bytes)
#pragma unroll
    for (int k = 0; k < PER; ++k) L.rgba[(size_t)slot * VOX + threadIdx.x + T * k] = col[k];
  }
}

}  // namespace vgx

using namespace vgx;

namespace {

int fail_fn(vgx_ctx ctx, int code, const char* fn, const std::string& msg) { return set_error(ctx, code, fn + msg); }

// vgx_tsdf_layer_merge_submaps (copy = false) and vgx_tsdf_layer_transform_submap (copy = true, n = 1): one pair build,
// one sort, one reservation; the copy additionally refuses a layer that is not empty
int project_submaps(vgx_tsdf_layer L, int32_t n, const vgx_submap* submaps, const float* T_L_S, int64_t* n_blocks_out,
                    bool copy, const char* kFn) {
  auto fail = [kFn](vgx_ctx c, int code, const std::string& msg) { return fail_fn(c, code, kFn, msg); };
  if (!L) return VGX_ERR_INVALID;
  vgx_ctx ctx = L->ctx;
  if (n < 0) return fail(ctx, VGX_ERR_INVALID, "n < 0");
  if (n > 0 && (!submaps || !T_L_S)) return fail(ctx, VGX_ERR_INVALID, "NULL submaps / T_L_S with n > 0");
  const TsdfLayerDev& ld = L->dev;
  for (int32_t i = 0; i < n; ++i) {
    const vgx_submap sm = submaps[i];
    const std::string at = "submap " + std::to_string(i) + ": ";
    if (!sm || sm->ctx != ctx) return fail(ctx, VGX_ERR_INVALID, at + "NULL or of another context");
    if (sm->voxel_size != ld.voxel_size || sm->vps != ld.vps)
      return fail(ctx, VGX_ERR_INVALID, at + "voxel_size / voxels_per_side differ from the layer's (no resampling)");
    if (sm->n_blocks > 0 && (!sm->d_tsdf_distance || !sm->d_tsdf_weight))
      return fail(ctx, VGX_ERR_INVALID, at + "raw TSDF layer not resident (released?)");
    const PoseDefect bad = pose_defect(T_L_S + 7 * (size_t)i);
    if (bad == kPoseNotFinite) return fail(ctx, VGX_ERR_INVALID, at + "pose value not finite");
    if (bad == kPoseNotUnit) return fail(ctx, VGX_ERR_INVALID, at + "pose quaternion not unit (|q|^2 - 1 > 1e-4)");
  }
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);  // (lock order: tsdf_mu, then mu)
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int32_t nb_now = 0;
  unsigned long long dropped = 0;
  if (copy) {
    int rc = tsdf_read_stats(L, &nb_now, &dropped);
    if (rc != VGX_OK) return rc;
    if (nb_now != 0) return fail(ctx, VGX_ERR_INVALID, "the layer is not empty (transformLayer writes into an empty layer)");
  }
  if (n == 0) {
    if (n_blocks_out) {
      int rc = tsdf_read_stats(L, &nb_now, &dropped);
      if (rc != VGX_OK) return rc;
      *n_blocks_out = nb_now;
    }
    return VGX_OK;
  }
  const int vps = ld.vps;
  const float bs = (float)vps * ld.voxel_size, bs_inv = 1.0f / bs;

  // 1. block flags (registration stream: where submap layers are produced), then the TSDF stream waits for them
  std::vector<ProjectSrc> src((size_t)n);
  std::vector<int64_t> src_first((size_t)n + 1, 0);
  int64_t box_lo[3] = {0, 0, 0}, box_hi[3] = {-1, -1, -1};
  bool any_box = false, any_colors = false;
  for (int32_t i = 0; i < n; ++i) {
    vgx_submap sm = submaps[i];
    if (sm->n_blocks > 0 && !sm->d_block_has_data) {
      VGX_HIP(ctx, sm->d_block_has_data.alloc_n((size_t)sm->n_blocks));
      if (vps == 16)
        hipLaunchKernelGGL(block_has_data_kernel<16>, dim3((unsigned)sm->n_blocks), dim3(256), 0, ctx->stream, sm->d_tsdf_weight,
                           sm->d_block_has_data);
      else
        hipLaunchKernelGGL(block_has_data_kernel<8>, dim3((unsigned)sm->n_blocks), dim3(256), 0, ctx->stream, sm->d_tsdf_weight,
                           sm->d_block_has_data);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) {
        sm->d_block_has_data.release();
        return fail(ctx, VGX_ERR_HIP, std::string("flag kernel: ") + hipGetErrorString(e));
      }
    }
    ProjectSrc& s = src[(size_t)i];
    static_cast<LayerTable&>(s) = submap_table(sm);
    s.tsdf_d = sm->d_tsdf_distance;
    s.tsdf_w = sm->d_tsdf_weight;
    s.block_index = sm->d_block_index;
    s.has_data = sm->d_block_has_data;
    s.tsdf_rgba = sm->d_tsdf_rgba;
    any_colors = any_colors || sm->d_tsdf_rgba != nullptr;
    const float* T = T_L_S + 7 * (size_t)i;
    for (int k = 0; k < 4; ++k) s.q_ls[k] = T[k];
    for (int k = 0; k < 3; ++k) s.t_ls[k] = T[4 + k];
    inverse_pose(s.q_ls, s.t_ls, s.q_sl, s.t_sl);
    src_first[(size_t)i + 1] = src_first[(size_t)i] + sm->n_blocks;
    if (sm->n_blocks == 0) continue;
    // candidate box: the submap's whole block box, grown by a voxel, into the layer frame, plus a block of slack
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
      int32_t lo = sm->block_index[(size_t)a], hi = lo;
      for (int32_t b = 1; b < sm->n_blocks; ++b) {
        lo = std::min(lo, sm->block_index[3 * (size_t)b + a]);
        hi = std::max(hi, sm->block_index[3 * (size_t)b + a]);
      }
      mn[a] = (float)lo * sm->block_size - sm->voxel_size;
      mx[a] = (float)(hi + 1) * sm->block_size + sm->voxel_size;
    }
    for (int k = 0; k < 8; ++k) {
      const float c[3] = {(k & 1) ? mx[0] : mn[0], (k & 2) ? mx[1] : mn[1], (k & 4) ? mx[2] : mn[2]};
      float g[3];
      rigid_apply(s.q_ls, s.t_ls, c, g);
      for (int a = 0; a < 3; ++a) {
        const int64_t lo = (int64_t)std::floor((double)g[a] * bs_inv) - 1, hi = (int64_t)std::floor((double)g[a] * bs_inv) + 1;
        if (!any_box || lo < box_lo[a]) box_lo[a] = lo;
        if (!any_box || hi > box_hi[a]) box_hi[a] = hi;
      }
      any_box = true;
    }
  }
  const int64_t total_blocks = src_first[(size_t)n];
  if (!any_box || total_blocks == 0) {
    int rc = tsdf_read_stats(L, &nb_now, &dropped);
    if (rc == VGX_OK && n_blocks_out) *n_blocks_out = nb_now;
    return rc;
  }
  // key = (cell of the target block in the candidate box) << pos_bits | array position
  int pos_bits = 1;
  while ((1ll << pos_bits) < (int64_t)n) ++pos_bits;
  double cells = 1.0;
  int32_t blo[3], bdim[3];
  for (int a = 0; a < 3; ++a) {
    const int64_t dm = box_hi[a] - box_lo[a] + 1;
    if (box_lo[a] < INT32_MIN / 2 || box_hi[a] > INT32_MAX / 2 || dm > (1ll << 28))
      return fail(ctx, VGX_ERR_UNSUPPORTED, "submaps too far apart (candidate block box)");
    blo[a] = (int32_t)box_lo[a];
    bdim[a] = (int32_t)dm;
    cells *= (double)dm;
  }
  if (cells * std::ldexp(1.0, pos_bits) >= std::ldexp(1.0, 63))
    return fail(ctx, VGX_ERR_UNSUPPORTED, "candidate block box too large for 64-bit keys");
  unsigned end_bit = (unsigned)pos_bits;
  while (std::ldexp(1.0, (int)end_bit - pos_bits) < cells) ++end_bit;
  const int3 box_lo3 = make_int3(blo[0], blo[1], blo[2]), box_dim3 = make_int3(bdim[0], bdim[1], bdim[2]);

  hipStream_t st = ctx->tsdf_stream;
  {
    hipEvent_t ev = nullptr;
    VGX_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
    (void)hipEventDestroy(ev);
    VGX_HIP(ctx, e);
  }

  // 2. candidate pairs: count, then emit
  DeviceBuffer d_src, d_first, d_cursor;
  VGX_HIP(ctx, d_src.alloc(src.size() * sizeof(ProjectSrc)));
  VGX_HIP(ctx, d_first.alloc(src_first.size() * sizeof(int64_t)));
  VGX_HIP(ctx, d_cursor.alloc(sizeof(unsigned long long)));
  VGX_HIP(ctx, hipMemcpyAsync(d_src.p, src.data(), src.size() * sizeof(ProjectSrc), hipMemcpyHostToDevice, st));
  VGX_HIP(ctx, hipMemcpyAsync(d_first.p, src_first.data(), src_first.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  VGX_HIP(ctx, hipMemsetAsync(d_cursor.p, 0, sizeof(unsigned long long), st));
  const unsigned pair_grid = (unsigned)((total_blocks + 255) / 256);
  hipLaunchKernelGGL(project_pairs_kernel, dim3(pair_grid), dim3(256), 0, st, d_src.as<ProjectSrc>(), d_first.as<int64_t>(), (int)n,
                     total_blocks, box_lo3, box_dim3, pos_bits, (unsigned long long*)nullptr, d_cursor.as<unsigned long long>(), 0ull);
  VGX_HIP(ctx, hipGetLastError());
  unsigned long long n_pairs64 = 0;
  VGX_HIP(ctx, hipMemcpyAsync(&n_pairs64, d_cursor.p, sizeof(n_pairs64), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  if (n_pairs64 >= (1ull << 31)) return fail(ctx, VGX_ERR_UNSUPPORTED, "more than 2^31 candidate (block, submap) pairs");
  const uint32_t n_pairs = (uint32_t)n_pairs64;
  if (n_pairs == 0) {
    int rc = tsdf_read_stats(L, &nb_now, &dropped);
    if (rc == VGX_OK && n_blocks_out) *n_blocks_out = nb_now;
    return rc;
  }
  DeviceBuffer d_keys, d_sorted, d_heads, d_seg, d_nseg, d_tmp;
  VGX_HIP(ctx, d_keys.alloc((size_t)n_pairs * 8));
  VGX_HIP(ctx, d_sorted.alloc((size_t)n_pairs * 8));
  VGX_HIP(ctx, d_heads.alloc((size_t)n_pairs));
  VGX_HIP(ctx, d_seg.alloc((size_t)n_pairs * 4));
  VGX_HIP(ctx, d_nseg.alloc(sizeof(uint32_t)));
  VGX_HIP(ctx, hipMemsetAsync(d_cursor.p, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(project_pairs_kernel, dim3(pair_grid), dim3(256), 0, st, d_src.as<ProjectSrc>(), d_first.as<int64_t>(), (int)n,
                     total_blocks, box_lo3, box_dim3, pos_bits, d_keys.as<unsigned long long>(), d_cursor.as<unsigned long long>(),
                     (unsigned long long)n_pairs);
  VGX_HIP(ctx, hipGetLastError());

  // 3. sort; segment starts.  The two share d_tmp and queue back to back: room for the larger is made once, before the sort
  auto sort = [&](void* tmp, size_t& bytes) {
    return rocprim::radix_sort_keys(tmp, bytes, d_keys.as<unsigned long long>(), d_sorted.as<unsigned long long>(), (size_t)n_pairs, 0u,
                                    end_bit, st);
  };
  auto select = [&](void* tmp, size_t& bytes) {
    return rocprim::select(tmp, bytes, rocprim::make_counting_iterator<uint32_t>(0u), d_heads.as<uint8_t>(), d_seg.as<uint32_t>(),
                           d_nseg.as<uint32_t>(), (size_t)n_pairs, st);
  };
  size_t sort_bytes = 0, select_bytes = 0;
  VGX_HIP(ctx, temp_bytes(sort, &sort_bytes));
  VGX_HIP(ctx, temp_bytes(select, &select_bytes));
  VGX_HIP(ctx, d_tmp.alloc(std::max<size_t>(std::max(sort_bytes, select_bytes), 4)));
  VGX_HIP(ctx, sort(d_tmp.p, sort_bytes));
  hipLaunchKernelGGL(segment_heads_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, st, d_sorted.as<unsigned long long>(), n_pairs,
                     pos_bits, d_heads.as<uint8_t>());
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, select(d_tmp.p, select_bytes));
  uint32_t n_seg = 0;
  VGX_HIP(ctx, hipMemcpyAsync(&n_seg, d_nseg.p, sizeof(n_seg), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));

  // 4. room for every candidate block (before any voxel is touched), then the merge
  const int32_t hi3[3] = {blo[0] + bdim[0] - 1, blo[1] + bdim[1] - 1, blo[2] + bdim[2] - 1};
  int rc = tsdf_reserve_blocks(L, blo, hi3, (int64_t)n_seg);
  if (rc != VGX_OK) return rc;
  if (n_seg > 0) {
    // the colour variant only when a submap of the call has colours
    auto kernel = vps == 16 ? (copy ? project_merge_kernel<16, 4, true, false> : project_merge_kernel<16, 4, false, false>)
                            : (copy ? project_merge_kernel<8, 2, true, false> : project_merge_kernel<8, 2, false, false>);
    if (any_colors)
      kernel = vps == 16 ? (copy ? project_merge_kernel<16, 4, true, true> : project_merge_kernel<16, 4, false, true>)
                         : (copy ? project_merge_kernel<8, 2, true, true> : project_merge_kernel<8, 2, false, true>);
    hipLaunchKernelGGL(kernel, dim3(n_seg), dim3(vps == 16 ? 1024 : 256), 0, st, d_sorted.as<unsigned long long>(),
                       d_seg.as<uint32_t>(), n_pairs, d_src.as<ProjectSrc>(), L->dev, box_lo3, box_dim3, pos_bits);
    VGX_HIP(ctx, hipGetLastError());
  }
  // the sources have been read once the stream is drained (tsdf_read_stats waits for it): the caller may destroy them
  rc = tsdf_read_stats(L, &nb_now, &dropped);
  if (rc != VGX_OK) return rc;
  if (dropped != 0) return fail(ctx, VGX_ERR_NOMEM, std::to_string(dropped) + " voxel updates dropped (allocation failed)");
  if (n_blocks_out) *n_blocks_out = nb_now;
  return VGX_OK;
}

}  // namespace

extern "C" int vgx_tsdf_layer_merge_submaps(vgx_tsdf_layer L, int32_t n, const vgx_submap* submaps, const float* T_L_S,
                                            int64_t* n_blocks_out) {
  return project_submaps(L, n, submaps, T_L_S, n_blocks_out, false, "vgx_tsdf_layer_merge_submaps: ");
}

extern "C" int vgx_tsdf_layer_transform_submap(vgx_tsdf_layer L, vgx_submap submap, const float T_L_S[7], int64_t* n_blocks_out) {
  if (!L) return VGX_ERR_INVALID;
  if (!submap || !T_L_S) return set_error(L->ctx, VGX_ERR_INVALID, "vgx_tsdf_layer_transform_submap: NULL submap / T_L_S");
  return project_submaps(L, 1, &submap, T_L_S, n_blocks_out, true, "vgx_tsdf_layer_transform_submap: ");
}
