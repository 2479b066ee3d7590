// Trilinear interpolation on a submap's raw TSDF or ESDF layer (device side).  gfx950 only.
#ifndef VGX_INTERP_H_
#define VGX_INTERP_H_

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#pragma clang fp contract(off)

namespace vgx {

// Interpolator<VoxelType>::getVoxelsAndQVector [recalled], split so that a caller can form the indices of several
// interpolations before it reads any voxel (vgx_query.hip): blk / vox the low neighbour's block and voxel index, dl the
// position within the cube in voxels.  P carries voxel_size, voxel_size_inv, block_size, block_size_inv.
template <int VPS, class P>
__device__ __forceinline__ void interp_base(const P& p, const float pos[3], int blk[3], int vox[3], float dl[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int b0 = (int)floorf(pos[a] * p.block_size_inv + 1e-6f);
    float origin = (float)b0 * p.block_size;
    int v = (int)floorf((pos[a] - origin) * p.voxel_size_inv + 1e-6f);
    v = min(max(v, 0), VPS - 1);
    float centre = origin + ((float)v + 0.5f) * p.voxel_size;
    // setIndexes: the block containing pos must exist (checked by the caller through neighbours: it is the block of
    // one of the 8 neighbours)
    if (pos[a] - centre < 0.0f) {
      v--;
      if (v < 0) {
        b0--;
        v += VPS;
      }
    }
    float origin2 = (float)b0 * p.block_size;
    dl[a] = (pos[a] - (origin2 + ((float)v + 0.5f) * p.voxel_size)) * p.voxel_size_inv;
    blk[a] = b0;
    vox[a] = v;
  }
}

// the block's slot through the dense lookup table (P: lut, lut_min / lut_dim as int3), -1 when absent.  (layer_interp keeps
// its own copy of these lines: routed through this function, the projected-map kernels took two more VGPRs.)
template <class P>
__device__ __forceinline__ int interp_slot(const P& p, int bx, int by, int bz) {
  int rx = bx - p.lut_min.x, ry = by - p.lut_min.y, rz = bz - p.lut_min.z;
  if ((unsigned)rx >= (unsigned)p.lut_dim.x || (unsigned)ry >= (unsigned)p.lut_dim.y || (unsigned)rz >= (unsigned)p.lut_dim.z)
    return -1;
  return p.lut[rx + p.lut_dim.x * (ry + p.lut_dim.y * rz)];
}

// The neighbour walk: the 8 neighbours of the low neighbour (blk, vox) (k: x = bit 2, y = bit 1, z = bit 0, a voxel index
// past the block carrying into the next block), each as its voxel's offset at[k] into a [slot][VPS^3] array.  False when
// a neighbour's block is absent; its at[k] is then formed with slot 0, so that a caller may form all 8 before it looks.
template <int VPS, class P>
__device__ __forceinline__ bool interp_neighbours(const P& p, const int blk[3], const int vox[3], size_t at[8]) {
  constexpr int VOX = VPS * VPS * VPS;
  bool ok = true;
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
    const int slot = interp_slot(p, nb[0], nb[1], nb[2]);
    ok = ok && slot >= 0;
    at[k] = (size_t)(slot >= 0 ? slot : 0) * VOX + (size_t)(nv[0] + VPS * (nv[1] + VPS * nv[2]));
  }
  return ok;
}

// interpVoxel's trilinear form over the 8 neighbours (k: x = bit 2, y = bit 1, z = bit 0) in oracle/iso_oracle.c's
// association
__device__ __forceinline__ float interp_trilinear(const float x[8], const float dl[3]) {
  float c0 = x[0], c1 = -x[0] + x[4], c2 = -x[0] + x[2], c3 = -x[0] + x[1];
  float c4 = ((x[0] - x[2]) - x[4]) + x[6];
  float c5 = ((x[0] - x[1]) - x[2]) + x[3];
  float c6 = ((x[0] - x[1]) - x[4]) + x[5];
  float c7 = ((((((-x[0] + x[1]) + x[2]) - x[3]) + x[4]) - x[5]) - x[6]) + x[7];
  float q4 = dl[0] * dl[1], q5 = dl[1] * dl[2], q6 = dl[2] * dl[0], q7 = dl[0] * dl[1] * dl[2];
  return ((((((c0 + dl[0] * c1) + dl[1] * c2) + dl[2] * c3) + q4 * c4) + q5 * c5) + q6 * c6) + q7 * c7;
}

// The exact derivative of interp_trilinear's form with respect to dl (in voxels), from the same 8 values and in the same
// coefficients; every sum left to right.  Defined here (scan-to-map registration, vgx_scan_reg.hip): voxblox has no
// counterpart, its gradients are central differences of seven interpolations.
__device__ __forceinline__ void interp_trilinear_gradient(const float x[8], const float dl[3], float g[3]) {
  float c1 = -x[0] + x[4], c2 = -x[0] + x[2], c3 = -x[0] + x[1];
  float c4 = ((x[0] - x[2]) - x[4]) + x[6];
  float c5 = ((x[0] - x[1]) - x[2]) + x[3];
  float c6 = ((x[0] - x[1]) - x[4]) + x[5];
  float c7 = ((((((-x[0] + x[1]) + x[2]) - x[3]) + x[4]) - x[5]) - x[6]) + x[7];
  g[0] = ((c1 + dl[1] * c4) + dl[2] * c6) + (dl[1] * dl[2]) * c7;
  g[1] = ((c2 + dl[0] * c4) + dl[2] * c5) + (dl[2] * dl[0]) * c7;
  g[2] = ((c3 + dl[1] * c5) + dl[0] * c6) + (dl[0] * dl[1]) * c7;
}

// Interpolator<VoxelType>::isVoxelValid on the layer's validity array: TSDF weight > 0, ESDF observed != 0
__device__ __forceinline__ bool interp_valid(float w) { return w > 0.0f; }
__device__ __forceinline__ bool interp_valid(uint8_t o) { return o != 0; }

// Interpolator<VoxelType>::getVoxel(p, &v, true) [recalled], i.e. getVoxelsAndQVector + interpVoxel, on one raw layer
// ([n_blocks][VPS^3] values and validity, voxblox linear voxel order, blocks found through a dense lookup table): false
// unless all 8 neighbours exist and are valid; then the value interpolated and -- for a TSDF layer, whose validity array
// is the weight -- the weight too (`wgt` is left alone for an ESDF layer).
template <int VPS, class P, class V>
__device__ bool layer_interp(const P& p, const float* val, const V* vld, const float pos[3], float& dist, float& wgt) {
  constexpr bool kTsdf = sizeof(V) == sizeof(float);
  constexpr int VOX = VPS * VPS * VPS;
  int blk[3], vox[3];
  float dl[3];
  interp_base<VPS>(p, pos, blk, vox, dl);
  float d[8], w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int off[3] = {(k >> 2) & 1, (k >> 1) & 1, k & 1};
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
    int rx = nb[0] - p.lut_min.x, ry = nb[1] - p.lut_min.y, rz = nb[2] - p.lut_min.z;
    if ((unsigned)rx >= (unsigned)p.lut_dim.x || (unsigned)ry >= (unsigned)p.lut_dim.y ||
        (unsigned)rz >= (unsigned)p.lut_dim.z)
      return false;
    int slot = p.lut[rx + p.lut_dim.x * (ry + p.lut_dim.y * rz)];
    if (slot < 0) return false;
    size_t at = (size_t)slot * VOX + (size_t)(nv[0] + VPS * (nv[1] + VPS * nv[2]));
    d[k] = val[at];
    const V v = vld[at];
    if (kTsdf) w[k] = (float)v;
    if (!interp_valid(v)) return false;  // Interpolator<VoxelType>::isVoxelValid
  }
  auto interp = [&](const float x[8]) { return interp_trilinear(x, dl); };
  dist = interp(d);
  if (kTsdf) wgt = interp(w);
  return true;
}

// Interpolator<TsdfVoxel>::getVoxel(p, &v, true) on a submap's raw TSDF layer: layer_interp over distance and weight.
// P carries lut, lut_min / lut_dim (int3), tsdf_d, tsdf_w, voxel_size, voxel_size_inv, block_size, block_size_inv.
// Shared by the isosurface points (vgx_iso.hip), the projected map (vgx_project.hip) and the map queries
// (vgx_query.hip); the first two are pinned to the oracle bit for bit, so this is the one copy.
template <int VPS, class P>
__device__ bool tsdf_interp(const P& p, const float pos[3], float& dist, float& wgt) {
  return layer_interp<VPS>(p, p.tsdf_d, p.tsdf_w, pos, dist, wgt);
}

// Interpolator<TsdfVoxel>::interpVoxel's colour [recalled] at a point where tsdf_interp returned true (all 8 neighbours
// exist): per channel the 8 neighbours' bytes widened to f32, in layer_interp's neighbour order, through interp_trilinear
// with the same dl as distance and weight.  voxblox assigns that float to a uint8_t member; here it is clamped to [0, 255]
// first and then truncated toward zero -- a stated definition for the few-ulp overshoots the C++ cast leaves undefined.
// rgba: [n_blocks][VPS^3] words, bytes r g b a (r lowest).  A pass of its own, after tsdf_interp, so that the 8 colour
// words are not live next to the 16 distance / weight values.
template <int VPS, class P>
__device__ __forceinline__ uint32_t tsdf_color_interp(const P& p, const uint32_t* __restrict__ rgba, const float pos[3]) {
  int blk[3], vox[3];
  float dl[3];
  interp_base<VPS>(p, pos, blk, vox, dl);
  size_t at[8];
  const bool all = interp_neighbours<VPS>(p, blk, vox, at);  // (true: the caller checked)
  uint32_t c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = all ? rgba[at[k]] : 0u;
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (float)((c[k] >> (8 * ch)) & 0xffu);
    const float v = fminf(fmaxf(interp_trilinear(x, dl), 0.0f), 255.0f);
    out |= (uint32_t)v << (8 * ch);
  }
  return out;
}

}  // namespace vgx

#endif  // VGX_INTERP_H_
