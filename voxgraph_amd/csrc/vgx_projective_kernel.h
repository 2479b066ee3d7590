// The block walk of the projective integrators, generic over the frame: the depth-image frame
// (vgx_projective.hip) and the LiDAR range-image frame (vgx_range_image.hip) instantiate it.  A frame type derives from
// ProjFrameBase and supplies
//   bool term(c, voxel_size, vx, vy, vz, sdf, uw, color, kind)   what the frame does to a voxel: false = no update; else the
//        update's sdf, weight and colour, and kind = 0 inside the truncation band or behind the surface, 1 carved, 2 cleared
//   bool block_in_view(block_size, bx, by, bz)                    can any voxel of the block find a pixel?  (conservative:
//        true when in doubt)
// gfx950 only.
#ifndef VGX_PROJECTIVE_KERNEL_H_
#define VGX_PROJECTIVE_KERNEL_H_

#include <string>

#include "vgx_internal.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

// u64 words of vgx_tsdf_integrator_s::d_proj_ctl
enum { kProjTicket = 0, kProjError = 1, kProjNew = 2, kProjUpdates = 3, kProjCarved = 4, kProjCleared = 5, kProjDropped = 6,
       kProjCtlWords = 8 };
constexpr int kProjThreads = 512;  // lanes of a workgroup: one block of 8^3 voxels, an eighth of one of 16^3
constexpr int64_t kProjMaxCandidates = (int64_t)1 << 24;

struct ProjFrameBase {
  float qw, qx, qy, qz, tx, ty, tz;  // T_G_C
  int32_t lo[3], nx, ny;  // the candidate box: its first block and its extent along x and y
  uint32_t tiles;         // candidates
  int32_t base_blocks;    // blocks the layer holds before the frame
};

// the inverse of T_G_C applied to a layer-frame point: subtract the translation, then rotate by the conjugate quaternion
// in transform_point's operation order (uv = qv x p, uv += uv, cc = qv x uv, p + qw uv + cc with qv = -(qx, qy, qz))
__device__ __forceinline__ void to_camera(const ProjFrameBase& f, float gx, float gy, float gz, float& x, float& y, float& z) {
  const float px = gx - f.tx, py = gy - f.ty, pz = gz - f.tz;
  const float qx = -f.qx, qy = -f.qy, qz = -f.qz;
  float uvx = qy * pz - qz * py, uvy = qz * px - qx * pz, uvz = qx * py - qy * px;
  uvx += uvx; uvy += uvy; uvz += uvz;
  const float ccx = qy * uvz - qz * uvy, ccy = qz * uvx - qx * uvz, ccz = qx * uvy - qy * uvx;
  x = px + f.qw * uvx + ccx;
  y = py + f.qw * uvy + ccy;
  z = pz + f.qw * uvz + ccz;
}

// the centre of block (bx, by, bz) in the camera frame, and the radius of the sphere around the block's voxel centres,
// 2 % wider, plus 1e-5 of every magnitude that went into a coordinate (f32: 6e-8 per operation, a dozen operations)
__device__ __forceinline__ float block_sphere(const ProjFrameBase& f, float block_size, int bx, int by, int bz, float& x, float& y,
                                              float& z) {
  const float gx = ((float)bx + 0.5f) * block_size, gy = ((float)by + 0.5f) * block_size, gz = ((float)bz + 0.5f) * block_size;
  to_camera(f, gx, gy, gz, x, y, z);
  return 0.8660254f * block_size * 1.02f + 1e-5f * (fabsf(gx) + fabsf(gy) + fabsf(gz) + fabsf(f.tx) + fabsf(f.ty) + fabsf(f.tz));
}

template <class Frame, int VPS>
__global__ __launch_bounds__(kProjThreads) void projective_kernel(TsdfLayerDev L, vgx_tsdf_config c, Frame f, TileChain chain,
                                                                  unsigned long long* __restrict__ ctl) {
  constexpr int kShift = VPS == 16 ? 4 : 3, kMask = VPS - 1, kVpb = VPS * VPS * VPS, kVpt = kVpb / kProjThreads;
  __shared__ uint32_t sh_word;
  const uint32_t tile = chain_tile(chain, &sh_word);
  // (tile < f.tiles: the launch has f.tiles workgroups and the ticket counts them)
  const int bx = f.lo[0] + (int)(tile % (uint32_t)f.nx);
  const int by = f.lo[1] + (int)((tile / (uint32_t)f.nx) % (uint32_t)f.ny);
  const int bz = f.lo[2] + (int)(tile / ((uint32_t)f.nx * (uint32_t)f.ny));
  // the block table covers the box (tsdf_reserve_blocks); a block outside it could only be dropped
  const int rx = bx - L.lut_min[0], ry = by - L.lut_min[1], rz = bz - L.lut_min[2];
  const bool in_table = (unsigned)rx < (unsigned)L.lut_dim[0] && (unsigned)ry < (unsigned)L.lut_dim[1] && (unsigned)rz < (unsigned)L.lut_dim[2];
  const size_t cell = in_table ? (size_t)rx + (size_t)L.lut_dim[0] * ((size_t)ry + (size_t)L.lut_dim[1] * (size_t)rz) : 0;
  int slot = in_table ? L.lut[cell] : -1;
  if (slot >= L.max_blocks) slot = -1;
  const bool present = slot >= 0;

  // A block the layer holds is updated in place; of an absent one only "does a voxel change" is kept, and the voxels
  // are formed again (a voxel of a fresh block is zero: nothing to load) once the block has its slot.
  uint32_t dirty_mask = 0, n_updates = 0, n_carved = 0, n_cleared = 0;
  if (f.block_in_view((float)VPS * L.voxel_size, bx, by, bz)) {
#pragma unroll 2
    for (int k = 0; k < kVpt; ++k) {
      const int v = k * kProjThreads + (int)threadIdx.x;
      const int lx = v & kMask, ly = (v >> kShift) & kMask, lz = v >> (2 * kShift);
      float sdf, uw;
      uint32_t color;
      int kind;
      if (!f.term(c, L.voxel_size, bx * VPS + lx, by * VPS + ly, bz * VPS + lz, sdf, uw, color, kind)) continue;
      float d = 0.0f, w = 0.0f;
      uint32_t col = 0u;
      const size_t at = (size_t)(present ? slot : 0) * kVpb + (size_t)v;
      if (present) {
        const unsigned long long old = L.voxels[at];
        d = __uint_as_float((unsigned)(old & 0xffffffffull));
        w = __uint_as_float((unsigned)(old >> 32));
        col = L.rgba[at];
      }
      bool dirty = false;
      apply_term(c, sdf, uw, color, d, w, col, dirty);
      if (!dirty) continue;
      if (present) {
        L.voxels[at] = pack_voxel(d, w);
        L.rgba[at] = col;
      }
      dirty_mask |= 1u << k;
      ++n_updates;
      n_carved += kind == 1;
      n_cleared += kind == 2;
    }
  }
  const bool any = __syncthreads_or(dirty_mask != 0u) != 0;
  const uint32_t needed = (!present && any) ? 1u : 0u;
  const uint32_t before = chain_exclusive_sum(chain, tile, needed, &sh_word);
  if (needed) {
    const long long s = (long long)f.base_blocks + (long long)before;
    slot = (in_table && s < (long long)L.max_blocks) ? (int)s : -1;
    if (slot >= 0) {
      if (threadIdx.x == 0) {
        L.block_index[3 * (size_t)slot + 0] = bx;
        L.block_index[3 * (size_t)slot + 1] = by;
        L.block_index[3 * (size_t)slot + 2] = bz;
        L.lut[cell] = slot;
      }
#pragma unroll 2
      for (int k = 0; k < kVpt; ++k) {
        if (!(dirty_mask & (1u << k))) continue;
        const int v = k * kProjThreads + (int)threadIdx.x;
        const int lx = v & kMask, ly = (v >> kShift) & kMask, lz = v >> (2 * kShift);
        float sdf, uw, d = 0.0f, w = 0.0f;
        uint32_t color, col = 0u;
        int kind;
        bool dirty = false;
        (void)f.term(c, L.voxel_size, bx * VPS + lx, by * VPS + ly, bz * VPS + lz, sdf, uw, color, kind);
        apply_term(c, sdf, uw, color, d, w, col, dirty);
        const size_t at = (size_t)slot * kVpb + (size_t)v;
        L.voxels[at] = pack_voxel(d, w);
        L.rgba[at] = col;
      }
    }
  }
  if (any) {
    // the frame's counters: a wave's sums, one atomic each (integer sums: the order does not show)
    uint32_t a = n_updates, b = n_carved, e = n_cleared;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      a += (uint32_t)__shfl_xor((int)a, d);
      b += (uint32_t)__shfl_xor((int)b, d);
      e += (uint32_t)__shfl_xor((int)e, d);
    }
    if ((threadIdx.x & 63) == 0 && a != 0u) {
      if (slot >= 0) {
        atomicAdd(ctl + kProjUpdates, (unsigned long long)a);
        if (b) atomicAdd(ctl + kProjCarved, (unsigned long long)b);
        if (e) atomicAdd(ctl + kProjCleared, (unsigned long long)e);
      } else {  // no room (cannot happen after tsdf_reserve_blocks): reported as the other integrators report it
        atomicAdd(ctl + kProjDropped, (unsigned long long)a);
        atomicAdd(L.dropped, (unsigned long long)a);
      }
    }
  }
  if (tile == f.tiles - 1u && threadIdx.x == 0) {
    const long long total = (long long)f.base_blocks + (long long)before + (long long)needed;
    *L.n_blocks = (int32_t)(total < (long long)L.max_blocks ? total : (long long)L.max_blocks);
    ctl[kProjNew] = (unsigned long long)(before + needed);
  }
}

template <class Frame>
void projective_launch(hipStream_t st, const TsdfLayerDev& L, const vgx_tsdf_config& c, const Frame& f, const TileChain& chain,
                       unsigned long long* ctl) {
  if (L.vps == 16)
    hipLaunchKernelGGL((projective_kernel<Frame, 16>), dim3(f.tiles), dim3(kProjThreads), 0, st, L, c, f, chain, ctl);
  else
    hipLaunchKernelGGL((projective_kernel<Frame, 8>), dim3(f.tiles), dim3(kProjThreads), 0, st, L, c, f, chain, ctl);
}

// ---- the host part the frames share (vgx_projective.hip); the caller holds the integrator's lock and ctx->tsdf_mu ----
// Room for every block of the candidate box [lo, hi] (tsdf_reserve_blocks: waits for the stream and reads the exact block
// count -- the frame's one host synchronisation), the control words and one chain word per candidate; fills the box fields
// of `f`.  VGX_OK or the code (error set, `fn` named).
int projective_begin(const char* fn, vgx_tsdf_integrator I, const int32_t lo[3], const int32_t hi[3], ProjFrameBase* f);
// right before the launch (nothing that can fail may come between): clears the frame's counters, takes the launch's epoch
// and tickets
int projective_chain(vgx_tsdf_integrator I, const ProjFrameBase& f, TileChain* chain);
// after the launch: notes the allocations; with counts the 56-byte read-back, and the call waits for the frame
int projective_end(const char* fn, vgx_tsdf_integrator I, const ProjFrameBase& f, vgx_projective_counts* counts);

}  // namespace vgx

#endif  // VGX_PROJECTIVE_KERNEL_H_
