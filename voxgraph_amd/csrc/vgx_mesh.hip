// The combined mesh on the device: voxblox::MeshIntegrator<TsdfVoxel>::generateMesh(false, false) [recalled] over a TSDF
// layer (a projected map, an active submap) or a finished submap's raw layer.  The semantics are stated in
// include/voxgraph_amd.h (vgx_tsdf_layer_generate_mesh); the layout and the passes in DESIGN.md 11.
//
//   1. order   the allocated blocks by block index: 64-bit keys (the block's cell in the dense block table, x-major) and
//              their slots, one radix sort
//   2. count   one workgroup per block in that order: the block's (vps+1)^3 corners staged in LDS (its own voxels and up
//              to 7 neighbour blocks through the table), per cube the configuration and its triangle count
//   3. scan    an inclusive scan of the counts gives every block's first triangle; the output grows once, to the total
//   4. emit    one workgroup per block again: the cubes in voxblox's visiting order, a workgroup-wide exclusive scan of
//              their counts per round of 256 cubes, each cube writing its triangles at its own offset.  No atomics on the
//              output: values and order do not depend on scheduling.
// The separated mesh (vgx_submaps_generate_separated_mesh) runs the same count and emit over every (submap,
// block) entry of n submaps at once: keys union_cell(block_index) * n + s, one sort, count (plus a flag where the block
// index changes), two scans, the unique blocks, one read-back, then emit with the submap's pose and colour applied just
// before the stores.  A fixed number of launches and two host synchronisations, whatever n.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "vgx_internal.h"
#include "vgx_mc_tables.h"
#include "vgx_pose.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

__constant__ int8_t c_mc_tri[256][16] = VGX_MC_TRIANGLE_TABLE;
__constant__ McCounts c_mc_count = mc_counts();

constexpr int kMeshThreads = 256;

// a TSDF source: the layer's packed {distance, weight} words or a submap's two raw arrays
struct MeshSrc {
  const int32_t* lut;  // dense [dim.z][dim.y][dim.x]: slot, or < 0
  int32_t lut_min[3], lut_dim[3];
  const int32_t* block_index;       // [slot][3]
  const unsigned long long* words;  // layer: [slot][vps^3]
  const float* dist;                // submap: [slot][vps^3]
  const float* weight;
  float voxel_size;
};

__device__ __forceinline__ int mesh_lookup(const MeshSrc& s, int bx, int by, int bz) {
  const int rx = bx - s.lut_min[0], ry = by - s.lut_min[1], rz = bz - s.lut_min[2];
  if ((unsigned)rx >= (unsigned)s.lut_dim[0] || (unsigned)ry >= (unsigned)s.lut_dim[1] || (unsigned)rz >= (unsigned)s.lut_dim[2])
    return -1;
  const int v = s.lut[rx + s.lut_dim[0] * (ry + s.lut_dim[1] * rz)];
  return v >= 0 ? v : -1;
}

// key = the block's cell in the table, x-major (ascending key = ascending (x, y, z))
__global__ __launch_bounds__(256) void mesh_keys_kernel(MeshSrc s, int32_t n, unsigned long long* __restrict__ keys,
                                                        int32_t* __restrict__ slots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t* b = s.block_index + 3 * (size_t)i;
  keys[i] = ((unsigned long long)(b[0] - s.lut_min[0]) * (unsigned long long)s.lut_dim[1] +
             (unsigned long long)(b[1] - s.lut_min[1])) * (unsigned long long)s.lut_dim[2] +
            (unsigned long long)(b[2] - s.lut_min[2]);
  slots[i] = i;
}

template <int VPS>
struct MeshLds {
  static constexpr int C = VPS + 1;
  float sdf[C * C * C];
  uint8_t ok[C * C * C];
  int nbr[8];
  int wave_sum[kMeshThreads / 64];
};

// the block's corners: voxel (cx, cy, cz) of [0, vps]^3, from the block or its +x / +y / +z neighbours
template <int VPS, bool PACKED>
__device__ __forceinline__ void stage_corners(const MeshSrc& s, int slot, const int32_t* bi, float min_weight, MeshLds<VPS>& m) {
  constexpr int C = VPS + 1, VOX = VPS * VPS * VPS;
  if (threadIdx.x < 8) {
    const int n = threadIdx.x;
    m.nbr[n] = n == 0 ? slot : mesh_lookup(s, bi[0] + (n & 1), bi[1] + ((n >> 1) & 1), bi[2] + ((n >> 2) & 1));
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * C * C; i += kMeshThreads) {
    const int cx = i % C, cy = (i / C) % C, cz = i / (C * C);
    const int n = (cx == VPS ? 1 : 0) | (cy == VPS ? 2 : 0) | (cz == VPS ? 4 : 0);
    const int lin = (cx & (VPS - 1)) + VPS * ((cy & (VPS - 1)) + VPS * (cz & (VPS - 1)));
    const int sl = m.nbr[n];
    float d = 0.0f;
    bool ok = false;
    if (sl >= 0) {
      float w;
      if (PACKED) {
        const unsigned long long v = s.words[(size_t)sl * VOX + lin];
        d = __uint_as_float((uint32_t)v);
        w = __uint_as_float((uint32_t)(v >> 32));
      } else {
        d = s.dist[(size_t)sl * VOX + lin];
        w = s.weight[(size_t)sl * VOX + lin];
      }
      ok = w > min_weight;  // utils::getSdfIfValid
    }
    m.sdf[i] = d;
    m.ok[i] = ok ? 1 : 0;
  }
  __syncthreads();
}

// corner i of the cube with low corner (x, y, z): cube_index_offsets_
__device__ __forceinline__ int corner_ox(int i) { return ((i + 1) >> 1) & 1; }  // 0 1 1 0 0 1 1 0
__device__ __forceinline__ int corner_oy(int i) { return (i >> 1) & 1; }        // 0 0 1 1 0 0 1 1
__device__ __forceinline__ int corner_oz(int i) { return (i >> 2) & 1; }        // 0 0 0 0 1 1 1 1

// configuration of the cube, or -1 when a corner is missing or too light
template <int VPS>
__device__ __forceinline__ int cube_config(const MeshLds<VPS>& m, int x, int y, int z, float sdf[8]) {
  constexpr int C = VPS + 1;
  int cfg = 0;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = (x + corner_ox(i)) + C * ((y + corner_oy(i)) + C * (z + corner_oz(i)));
    sdf[i] = m.sdf[idx];
    ok = ok && m.ok[idx];
    cfg |= sdf[i] < 0.0f ? (1 << i) : 0;
  }
  return ok ? cfg : -1;
}

// rank -> cube in voxblox's visiting order (extractBlockMesh)
template <int VPS>
__device__ __forceinline__ void visit(int r, int& x, int& y, int& z) {
  constexpr int M = VPS - 1;
  if (r < M * M * M) {
    x = r / (M * M);
    y = (r / M) % M;
    z = r % M;
    return;
  }
  r -= M * M * M;
  if (r < VPS * VPS) {
    x = M;
    z = r / VPS;
    y = r % VPS;
    return;
  }
  r -= VPS * VPS;
  if (r < VPS * M) {
    y = M;
    z = r / M;
    x = r % M;
    return;
  }
  r -= VPS * M;
  z = M;
  y = r / M;
  x = r % M;
}

// this thread's share of the block's triangle count (cubes r = threadIdx.x, + 256, ...)
template <int VPS>
__device__ __forceinline__ int thread_triangle_count(const MeshLds<VPS>& m) {
  int cnt = 0;
  for (int r = threadIdx.x; r < VPS * VPS * VPS; r += kMeshThreads) {
    float sdf[8];
    const int cfg = cube_config<VPS>(m, r % VPS, (r / VPS) % VPS, r / (VPS * VPS), sdf);
    if (cfg >= 0) cnt += c_mc_count.n[cfg];
  }
  return cnt;
}

template <int VPS, bool PACKED>
__global__ __launch_bounds__(kMeshThreads) void mesh_count_kernel(MeshSrc s, const int32_t* __restrict__ order, float min_weight,
                                                                   int64_t* __restrict__ counts, int32_t* __restrict__ out_bi) {
  __shared__ MeshLds<VPS> m;
  __shared__ int total;
  const int slot = order[blockIdx.x];
  const int32_t* bi = s.block_index + 3 * (size_t)slot;
  if (threadIdx.x == 0) total = 0;
  stage_corners<VPS, PACKED>(s, slot, bi, min_weight, m);
  atomicAdd(&total, thread_triangle_count<VPS>(m));  // (integer sum in LDS: exact in any order)
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = total;
    out_bi[3 * (size_t)blockIdx.x + 0] = bi[0];
    out_bi[3 * (size_t)blockIdx.x + 1] = bi[1];
    out_bi[3 * (size_t)blockIdx.x + 2] = bi[2];
  }
}

__device__ __forceinline__ void edge_vertex(const float pa[3], const float pb[3], float sa, float sb, float out[3]) {
  const float diff = sa - sb;
  if (fabsf(diff) >= 1e-6f) {
    const float t = sa / diff;
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = pa[a] + t * (pb[a] - pa[a]);
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) out[a] = 0.5f * (pa[a] + pb[a]);
  }
}

__device__ __forceinline__ void cube_edge_vertex(int e, const float base[3], float vs, const float sdf[8], float out[3]) {
  // kEdgeIndexPairs: 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7
  const int a = e < 8 ? e : e - 8;
  const int b = e < 8 ? ((e & 3) == 3 ? e - 3 : e + 1) : e - 4;
  const float pa[3] = {base[0] + (corner_ox(a) ? vs : 0.0f), base[1] + (corner_oy(a) ? vs : 0.0f), base[2] + (corner_oz(a) ? vs : 0.0f)};
  const float pb[3] = {base[0] + (corner_ox(b) ? vs : 0.0f), base[1] + (corner_oy(b) ? vs : 0.0f), base[2] + (corner_oz(b) ? vs : 0.0f)};
  edge_vertex(pa, pb, sdf[a], sdf[b], out);
}

// a rigid transform applied just before the stores (the separated mesh), or none
struct EmitPose {
  float q[4], t[3];  // T_M_S {w, x, y, z}, t
  uint32_t rgba;     // the triangle's colour, bytes r g b a
  uint32_t* colors;  // [T]
};

// One block's triangles at [base, end), its corners staged into m: the cubes in visiting order, a workgroup-wide exclusive
// scan of their counts per round of 256 cubes, each cube writing its triangles at its own offset.  POSED: each vertex
// through transform_point(T), the normal through the rotation alone (not renormalised), the colour stored per triangle.
template <int VPS, bool POSED>
__device__ __forceinline__ void emit_block(const MeshSrc& s, const int32_t* bi, int64_t base, int64_t end, MeshLds<VPS>& m,
                                           float* __restrict__ vertices, float* __restrict__ normals, const EmitPose& T) {
  constexpr int NW = kMeshThreads / 64;
  const float vs = s.voxel_size, bs = (float)VPS * vs;
  const float ox = (float)bi[0] * bs, oy = (float)bi[1] * bs, oz = (float)bi[2] * bs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r0 = 0; r0 < VPS * VPS * VPS; r0 += kMeshThreads) {
    int x, y, z;
    visit<VPS>(r0 + threadIdx.x, x, y, z);
    float sdf[8];
    const int cfg = cube_config<VPS>(m, x, y, z, sdf);
    const int n = cfg >= 0 ? (int)c_mc_count.n[cfg] : 0;
    // workgroup-wide exclusive prefix of n in visiting order
    int inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) m.wave_sum[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      before += w < wave ? m.wave_sum[w] : 0;
      all += m.wave_sum[w];
    }
    __syncthreads();  // (wave_sum is rewritten next round)
    int64_t at = base + before + inc - n;
    if (n > 0) {
      // Block::computeCoordinatesFromLinearIndex of the low voxel
      const float c[3] = {ox + ((float)x + 0.5f) * vs, oy + ((float)y + 0.5f) * vs, oz + ((float)z + 0.5f) * vs};
      for (int k = 0; k < n; ++k, ++at) {
        if (at >= end) break;  // (count and emit stage the same corners: not reached)
        float p[3][3];
        cube_edge_vertex(c_mc_tri[cfg][3 * k + 2], c, vs, sdf, p[0]);
        cube_edge_vertex(c_mc_tri[cfg][3 * k + 1], c, vs, sdf, p[1]);
        cube_edge_vertex(c_mc_tri[cfg][3 * k + 0], c, vs, sdf, p[2]);
        const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
        const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
        float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const float sq = (nx * nx + ny * ny) + nz * nz;
        if (sq > 0.0f) {
          const float len = sqrtf(sq);
          nx = nx / len;
          ny = ny / len;
          nz = nz / len;
        }
        if (POSED) {
#pragma unroll
          for (int q = 0; q < 3; ++q)
            transform_point(T.q[0], T.q[1], T.q[2], T.q[3], T.t[0], T.t[1], T.t[2], p[q][0], p[q][1], p[q][2], p[q][0], p[q][1],
                            p[q][2]);
          const float nrm[3] = {nx, ny, nz};
          float rot[3];
          quat_rotate(T.q, nrm, rot);  // (transform_point's formula up to its `+ t`)
          nx = rot[0];
          ny = rot[1];
          nz = rot[2];
          T.colors[at] = T.rgba;
        }
        float* v = vertices + 9 * at;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          v[3 * q + 0] = p[q][0];
          v[3 * q + 1] = p[q][1];
          v[3 * q + 2] = p[q][2];
        }
        normals[3 * at + 0] = nx;
        normals[3 * at + 1] = ny;
        normals[3 * at + 2] = nz;
      }
    }
    base += all;
  }
}

template <int VPS, bool PACKED>
__global__ __launch_bounds__(kMeshThreads) void mesh_emit_kernel(MeshSrc s, const int32_t* __restrict__ order, float min_weight,
                                                                  const int64_t* __restrict__ first, float* __restrict__ vertices,
                                                                  float* __restrict__ normals) {
  __shared__ MeshLds<VPS> m;
  const int slot = order[blockIdx.x];
  const int32_t* bi = s.block_index + 3 * (size_t)slot;
  stage_corners<VPS, PACKED>(s, slot, bi, min_weight, m);
  const int64_t end = first[blockIdx.x + 1];
  const int64_t base = first[blockIdx.x];
  const EmitPose none{};
  emit_block<VPS, false>(s, bi, base, end, m, vertices, normals, none);
}

// ---- the separated mesh (vgx_submaps_generate_separated_mesh): n submaps in one pass -------------------------------
// One entry per (submap, block), keyed by union_cell(block_index) * n + s: sorted, a block index's entries are
// consecutive and in array order.  DESIGN.md 13.

// one submap: its raw layer, its pose and colour, its first entry
struct SepSrc {
  MeshSrc m;
  EmitPose pose;  // (colors is the same for every submap: set on the device side of the copy)
  int64_t entry0;
};

// the union of the submaps' block tables
struct SepBox {
  long long lo[3];
  unsigned long long dim[3];
};

__global__ __launch_bounds__(256) void sep_keys_kernel(const SepSrc* __restrict__ src, int32_t n_src, int64_t n_entries, SepBox box,
                                                       unsigned long long* __restrict__ keys, int32_t* __restrict__ slots) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= n_entries) return;
  int a = 0, b = n_src;  // the last submap with entry0 <= g (an empty submap shares its entry0 with the next one)
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (src[m].entry0 <= g) a = m; else b = m;
  }
  const int32_t slot = (int32_t)(g - src[a].entry0);
  const int32_t* bi = src[a].m.block_index + 3 * (size_t)slot;
  const unsigned long long cell =
      ((unsigned long long)((long long)bi[0] - box.lo[0]) * box.dim[1] + (unsigned long long)((long long)bi[1] - box.lo[1])) * box.dim[2] +
      (unsigned long long)((long long)bi[2] - box.lo[2]);
  keys[g] = cell * (unsigned long long)n_src + (unsigned long long)a;
  slots[g] = slot;
}

// one workgroup per entry in key order: its triangle count, and whether it starts a new block index
template <int VPS>
__global__ __launch_bounds__(kMeshThreads) void sep_count_kernel(const SepSrc* __restrict__ src, unsigned long long n_src,
                                                                  const unsigned long long* __restrict__ keys,
                                                                  const int32_t* __restrict__ slots, float min_weight,
                                                                  int64_t* __restrict__ counts, int32_t* __restrict__ heads) {
  __shared__ MeshLds<VPS> m;
  __shared__ int total;
  const unsigned long long key = keys[blockIdx.x];
  const MeshSrc s = src[key % n_src].m;  // (uniform: one submap per workgroup)
  const int slot = slots[blockIdx.x];
  const int32_t* bi = s.block_index + 3 * (size_t)slot;
  if (threadIdx.x == 0) total = 0;
  stage_corners<VPS, false>(s, slot, bi, min_weight, m);
  atomicAdd(&total, thread_triangle_count<VPS>(m));  // (integer sum in LDS: exact in any order)
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = total;
    heads[blockIdx.x] = (blockIdx.x == 0 || keys[blockIdx.x - 1] / n_src != key / n_src) ? 1 : 0;
  }
}

// the block index of each head entry and the first triangle of its block; the last entry also writes first[nb] and
// tail = {triangles, blocks}
__global__ __launch_bounds__(256) void sep_unique_kernel(const SepSrc* __restrict__ src, unsigned long long n_src,
                                                         const unsigned long long* __restrict__ keys,
                                                         const int32_t* __restrict__ slots, int32_t n_entries,
                                                         const int32_t* __restrict__ heads, const int32_t* __restrict__ uid,
                                                         const int64_t* __restrict__ efirst, int32_t* __restrict__ out_bi,
                                                         int64_t* __restrict__ out_first, int64_t* __restrict__ tail) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_entries) return;
  if (heads[i]) {
    const int u = uid[i] - 1;
    const int32_t* bi = src[keys[i] % n_src].m.block_index + 3 * (size_t)slots[i];
    out_bi[3 * (size_t)u + 0] = bi[0];
    out_bi[3 * (size_t)u + 1] = bi[1];
    out_bi[3 * (size_t)u + 2] = bi[2];
    out_first[u] = efirst[i];
  }
  if (i == n_entries - 1) {
    out_first[uid[i]] = efirst[n_entries];
    tail[0] = efirst[n_entries];
    tail[1] = uid[i];
  }
}

// one workgroup per entry in key order: its triangles at [efirst[i], efirst[i+1]), posed and coloured
template <int VPS>
// (__launch_bounds__' second argument: at least 6 waves per SIMD, the LDS bound of MeshLds<16> -- no spill results)
__global__ __launch_bounds__(kMeshThreads, 6) void sep_emit_kernel(const SepSrc* __restrict__ src, unsigned long long n_src,
                                                                 const unsigned long long* __restrict__ keys,
                                                                 const int32_t* __restrict__ slots, float min_weight,
                                                                 const int64_t* __restrict__ efirst, float* __restrict__ vertices,
                                                                 float* __restrict__ normals, uint32_t* __restrict__ colors) {
  __shared__ MeshLds<VPS> m;
  const SepSrc& d = src[keys[blockIdx.x] % n_src];  // (uniform: one submap per workgroup)
  const MeshSrc s = d.m;
  EmitPose T = d.pose;
  T.colors = colors;
  const int64_t end = efirst[blockIdx.x + 1];
  const int64_t base = efirst[blockIdx.x];
  if (base == end) return;  // (no triangles: nothing to stage; uniform across the workgroup, before any barrier)
  const int slot = slots[blockIdx.x];
  const int32_t* bi = s.block_index + 3 * (size_t)slot;
  stage_corners<VPS, false>(s, slot, bi, min_weight, m);
  emit_block<VPS, true>(s, bi, base, end, m, vertices, normals, T);
}

// MeshIntegrator::updateMeshColor [recalled]: one thread per triangle of the soup, its three vertices coloured from the
// voxel each lies in.  k: the triangle's block (first[k] <= t < first[k + 1]) by bisection; the voxel index in that block is
// floorf((p - origin) * voxel_size_inv + 1e-6f) per axis; outside [0, VPS) on any axis (a vertex on the block's max
// planes) the block is floorf(p * block_size_inv + 1e-6f) and the index is recomputed against its origin and clamped
// (query_nearest's lines, vgx_query_kernel.h).  The colour word is copied when the voxel's weight >= min_weight
// (getColorIfValid); else, or when the block is absent (voxblox would dereference null), the vertex keeps (0, 0, 0, 0).
// A thread reads 36 contiguous bytes and writes 12; every output word has one writer.
template <int VPS, bool PACKED>
__global__ __launch_bounds__(256) void mesh_vertex_color_kernel(MeshSrc s, const uint32_t* __restrict__ rgba, float min_weight,
                                                                float voxel_size_inv, float block_size, float block_size_inv,
                                                                const int32_t* __restrict__ block_index, const int64_t* __restrict__ first,
                                                                int32_t n_blocks, int64_t n_tris, const float* __restrict__ vertices,
                                                                uint32_t* __restrict__ colors) {
  constexpr int VOX = VPS * VPS * VPS;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_tris) return;
  int lo = 0, hi = n_blocks;  // last k with first[k] <= t (first[0] = 0 <= t < first[n_blocks])
  while (hi - lo > 1) {
    const int m = (lo + hi) >> 1;
    if (first[m] <= t) lo = m; else hi = m;
  }
  const int b[3] = {block_index[3 * (size_t)lo], block_index[3 * (size_t)lo + 1], block_index[3 * (size_t)lo + 2]};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float p[3];
    int nb[3], v[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p[a] = vertices[9 * (size_t)t + 3 * c + a];
      nb[a] = b[a];
      const float origin = (float)b[a] * block_size;
      v[a] = (int)floorf((p[a] - origin) * voxel_size_inv + 1e-6f);
      inside = inside && (unsigned)v[a] < (unsigned)VPS;
    }
    if (!inside) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        nb[a] = (int)floorf(p[a] * block_size_inv + 1e-6f);
        const float origin = (float)nb[a] * block_size;
        v[a] = min(max((int)floorf((p[a] - origin) * voxel_size_inv + 1e-6f), 0), VPS - 1);
      }
    }
    uint32_t word = 0u;
    const int slot = mesh_lookup(s, nb[0], nb[1], nb[2]);
    if (slot >= 0) {
      const size_t at = (size_t)slot * VOX + (size_t)(v[0] + VPS * (v[1] + VPS * v[2]));
      const float w = PACKED ? __uint_as_float((uint32_t)(s.words[at] >> 32)) : s.weight[at];
      if (w >= min_weight) word = rgba[at];
    }
    colors[3 * (size_t)t + c] = word;
  }
}

}  // namespace vgx

using namespace vgx;

struct vgx_mesh_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  int32_t n_blocks = 0;  // the mesh held now
  int64_t n_tris = 0;
  bool holds_mesh = true;  // false from the moment a generating call resets the handle until one succeeds (vgx_mesh_connect)
  // output, grown on demand
  DeviceBuffer d_block_index;  // int32 [block_cap][3]
  DeviceBuffer d_first;        // int64 [block_cap + 1]
  DeviceBuffer d_vertices;     // float [tri_cap][3][3]
  DeviceBuffer d_normals;      // float [tri_cap][3]
  // per-block scratch
  DeviceBuffer d_keys[2];      // u64 [block_cap]
  DeviceBuffer d_slots[2];     // int32 [block_cap]
  DeviceBuffer d_counts;       // int64 [block_cap]
  DeviceBuffer d_tmp;          // rocPRIM's workspace: the largest any of a call's sorts and scans asks for
  // colours: one per triangle (the separated mesh) or, per_vertex, one per soup vertex (the _colored generators); the
  // separated mesh's per-entry scratch beside the block arrays, descriptors
  bool has_colors = false;
  bool per_vertex = false;
  DeviceBuffer d_colors;       // u32 [color_cap] bytes r g b a
  DeviceBuffer d_efirst;       // int64 [entry_cap + 1]
  DeviceBuffer d_heads;        // int32 [entry_cap]
  DeviceBuffer d_uid;          // int32 [entry_cap]
  DeviceBuffer d_tail;         // int64 {triangles, blocks}
  std::vector<SepSrc> h_src;   // (the host side of the descriptor copy: outlives it)
  DeviceBuffer d_src;          // SepSrc [src_cap]
  // a generating call starts from a handle that holds nothing
  void reset_stats() {
    n_blocks = 0;
    n_tris = 0;
    has_colors = false;
    per_vertex = false;
    holds_mesh = false;
  }
};

namespace {

// the block arrays (capacity: at least 1024 blocks, no slack) and the workspace, which goes when they go
int ensure_blocks(vgx_mesh M, int64_t nb, size_t tmp_bytes) {
  if ((size_t)nb * 8 > M->d_counts.bytes) {
    const size_t cap = (size_t)std::max<int64_t>(nb, 1024);
    M->d_tmp.release();
    const hipError_t e = alloc_group({{&M->d_block_index, cap * 12}, {&M->d_first, (cap + 1) * 8}, {&M->d_keys[0], cap * 8},
                                      {&M->d_slots[0], cap * 4}, {&M->d_keys[1], cap * 8}, {&M->d_slots[1], cap * 4},
                                      {&M->d_counts, cap * 8}});
    if (e != hipSuccess) return alloc_error(M->ctx, e, "mesh: allocating block arrays");
  }
  const hipError_t e = M->d_tmp.reserve(tmp_bytes);
  return e == hipSuccess ? VGX_OK : alloc_error(M->ctx, e, "mesh: allocating sort workspace");
}

// per-entry scratch (at least 1024 entries) and descriptors (at least 64); the block arrays come from ensure_blocks
int ensure_entries(vgx_mesh M, int64_t ne, int64_t n_src) {
  if ((size_t)ne * 4 > M->d_heads.bytes) {
    const size_t cap = (size_t)std::max<int64_t>(ne, 1024);
    const hipError_t e = alloc_group({{&M->d_efirst, (cap + 1) * 8}, {&M->d_heads, cap * 4}, {&M->d_uid, cap * 4},
                                      {&M->d_tail, 2 * sizeof(int64_t)}});
    if (e != hipSuccess) return alloc_error(M->ctx, e, "mesh: allocating entry arrays");
  }
  const hipError_t e = M->d_src.reserve((size_t)n_src * sizeof(SepSrc), 64 * sizeof(SepSrc));
  return e == hipSuccess ? VGX_OK : alloc_error(M->ctx, e, "mesh: allocating submap descriptors");
}

// a quarter of slack (the next map is a little larger), at least 4096 triangles
size_t tri_capacity(int64_t nt) { return (size_t)std::max<int64_t>(nt + nt / 4, 4096); }

int ensure_colors(vgx_mesh M, int64_t nt) {
  if ((size_t)nt * 4 <= M->d_colors.bytes) return VGX_OK;
  const hipError_t e = M->d_colors.alloc(tri_capacity(nt) * 4);
  return e == hipSuccess ? VGX_OK : alloc_error(M->ctx, e, "mesh: allocating colours");
}

int ensure_tris(vgx_mesh M, int64_t nt) {
  if ((size_t)nt * 12 <= M->d_normals.bytes) return VGX_OK;
  const size_t cap = tri_capacity(nt);
  const hipError_t e = alloc_group({{&M->d_vertices, cap * 36}, {&M->d_normals, cap * 12}});
  return e == hipSuccess ? VGX_OK : alloc_error(M->ctx, e, "mesh: allocating triangles");
}

template <bool PACKED>
hipError_t launch_count(int vps, hipStream_t st, int32_t nb, const MeshSrc& s, const int32_t* order, float mw, int64_t* counts,
                        int32_t* out_bi) {
  if (vps == 16)
    hipLaunchKernelGGL((mesh_count_kernel<16, PACKED>), dim3((unsigned)nb), dim3(kMeshThreads), 0, st, s, order, mw, counts, out_bi);
  else
    hipLaunchKernelGGL((mesh_count_kernel<8, PACKED>), dim3((unsigned)nb), dim3(kMeshThreads), 0, st, s, order, mw, counts, out_bi);
  return hipGetLastError();
}

template <bool PACKED>
hipError_t launch_emit(int vps, hipStream_t st, int32_t nb, const MeshSrc& s, const int32_t* order, float mw, const int64_t* first,
                       float* vert, float* norm) {
  if (vps == 16)
    hipLaunchKernelGGL((mesh_emit_kernel<16, PACKED>), dim3((unsigned)nb), dim3(kMeshThreads), 0, st, s, order, mw, first, vert, norm);
  else
    hipLaunchKernelGGL((mesh_emit_kernel<8, PACKED>), dim3((unsigned)nb), dim3(kMeshThreads), 0, st, s, order, mw, first, vert, norm);
  return hipGetLastError();
}

template <bool PACKED>
hipError_t launch_vertex_colors(int vps, hipStream_t st, const MeshSrc& s, const uint32_t* rgba, float mw, const int32_t* out_bi,
                                const int64_t* first, int32_t nb, int64_t total, const float* vert, uint32_t* colors) {
  // voxblox::Layer / Block constants, f32 [recalled] (vgx_submap_create)
  const float vsi = 1.0f / s.voxel_size, bs = (float)vps * s.voxel_size, bsi = 1.0f / bs;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (vps == 16)
    hipLaunchKernelGGL((mesh_vertex_color_kernel<16, PACKED>), grid, block, 0, st, s, rgba, mw, vsi, bs, bsi, out_bi, first, nb, total, vert,
                       colors);
  else
    hipLaunchKernelGGL((mesh_vertex_color_kernel<8, PACKED>), grid, block, 0, st, s, rgba, mw, vsi, bs, bsi, out_bi, first, nb, total, vert,
                       colors);
  return hipGetLastError();
}

// the passes, on `st` (the caller holds the source's locks and M->mu, and has reset M's stats).  rgba: the source's colour
// words ([slot][vps^3]) for one colour per soup vertex (the streaming pass queued behind the emit, before the one wait), or
// null: the plain mesh
template <bool PACKED>
int generate(vgx_ctx ctx, hipStream_t st, const MeshSrc& s, int vps, int32_t nb, float mw, vgx_mesh M, const uint32_t* rgba = nullptr) {
  if (nb == 0) return VGX_OK;
  double cells = 1.0;
  for (int a = 0; a < 3; ++a) cells *= (double)s.lut_dim[a];
  unsigned end_bit = 1;
  while (end_bit < 64 && std::ldexp(1.0, (int)end_bit) < cells) ++end_bit;
  // the sort and the scan share M->d_tmp and queue back to back: room for the larger is made once, before the first launch
  auto sort = [&](void* tmp, size_t& bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, M->d_keys[0].as<unsigned long long>(), M->d_keys[1].as<unsigned long long>(),
                                     M->d_slots[0].as<int32_t>(), M->d_slots[1].as<int32_t>(), (size_t)nb, 0u, end_bit, st);
  };
  auto scan = [&](void* tmp, size_t& bytes) {
    return rocprim::inclusive_scan(tmp, bytes, M->d_counts.as<int64_t>(), M->d_first.as<int64_t>() + 1, (size_t)nb,
                                   rocprim::plus<int64_t>(), st);
  };
  size_t sort_bytes = 0, scan_bytes = 0;
  VGX_HIP(ctx, temp_bytes(sort, &sort_bytes));
  VGX_HIP(ctx, temp_bytes(scan, &scan_bytes));
  int rc = ensure_blocks(M, nb, std::max<size_t>(std::max(sort_bytes, scan_bytes), 4));
  if (rc != VGX_OK) return rc;
  // 1. order
  hipLaunchKernelGGL(mesh_keys_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, s, nb, M->d_keys[0].as<unsigned long long>(),
                     M->d_slots[0].as<int32_t>());
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, sort(M->d_tmp.p, sort_bytes));
  // 2. count
  VGX_HIP(ctx, launch_count<PACKED>(vps, st, nb, s, M->d_slots[1].as<int32_t>(), mw, M->d_counts.as<int64_t>(),
                                    M->d_block_index.as<int32_t>()));
  // 3. scan
  VGX_HIP(ctx, hipMemsetAsync(M->d_first.p, 0, sizeof(int64_t), st));
  VGX_HIP(ctx, scan(M->d_tmp.p, scan_bytes));
  int64_t total = 0;
  VGX_HIP(ctx, hipMemcpyAsync(&total, M->d_first.as<int64_t>() + nb, sizeof(total), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  // 4. emit
  rc = ensure_tris(M, total);
  if (rc == VGX_OK && rgba) rc = ensure_colors(M, 3 * total);
  if (rc != VGX_OK) return rc;
  if (total > 0) {
    VGX_HIP(ctx, launch_emit<PACKED>(vps, st, nb, s, M->d_slots[1].as<int32_t>(), mw, M->d_first.as<int64_t>(), M->d_vertices.as<float>(),
                                     M->d_normals.as<float>()));
    if (rgba)
      VGX_HIP(ctx, launch_vertex_colors<PACKED>(vps, st, s, rgba, mw, M->d_block_index.as<int32_t>(), M->d_first.as<int64_t>(), nb, total,
                                                M->d_vertices.as<float>(), M->d_colors.as<uint32_t>()));
    VGX_HIP(ctx, hipStreamSynchronize(st));
  }
  M->n_blocks = nb;
  M->n_tris = total;
  return VGX_OK;
}

template <int VPS>
hipError_t launch_separated(bool emit, hipStream_t st, int32_t ne, vgx_mesh M, unsigned long long n_src, float mw) {
  if (emit)
    hipLaunchKernelGGL(sep_emit_kernel<VPS>, dim3((unsigned)ne), dim3(kMeshThreads), 0, st, M->d_src.as<SepSrc>(), n_src,
                       M->d_keys[1].as<unsigned long long>(), M->d_slots[1].as<int32_t>(), mw, M->d_efirst.as<int64_t>(),
                       M->d_vertices.as<float>(), M->d_normals.as<float>(), M->d_colors.as<uint32_t>());
  else
    hipLaunchKernelGGL(sep_count_kernel<VPS>, dim3((unsigned)ne), dim3(kMeshThreads), 0, st, M->d_src.as<SepSrc>(), n_src,
                       M->d_keys[1].as<unsigned long long>(), M->d_slots[1].as<int32_t>(), mw, M->d_counts.as<int64_t>(),
                       M->d_heads.as<int32_t>());
  return hipGetLastError();
}

// the separated passes over ne > 0 entries, on `st` (the caller holds the registration lock and M->mu, has reset M's
// stats and filled M->h_src)
int generate_separated(vgx_ctx ctx, hipStream_t st, int vps, int32_t ne, const SepBox& box, unsigned end_bit, float mw,
                       vgx_mesh M) {
  const int32_t n = (int32_t)M->h_src.size();
  // the sort and the two scans share M->d_tmp and queue back to back: room for the largest is made once, before the
  // first launch
  auto sort = [&](void* tmp, size_t& bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, M->d_keys[0].as<unsigned long long>(), M->d_keys[1].as<unsigned long long>(),
                                     M->d_slots[0].as<int32_t>(), M->d_slots[1].as<int32_t>(), (size_t)ne, 0u, end_bit, st);
  };
  auto scan = [&](void* tmp, size_t& bytes) {
    return rocprim::inclusive_scan(tmp, bytes, M->d_counts.as<int64_t>(), M->d_efirst.as<int64_t>() + 1, (size_t)ne,
                                   rocprim::plus<int64_t>(), st);
  };
  auto flag_scan = [&](void* tmp, size_t& bytes) {
    return rocprim::inclusive_scan(tmp, bytes, M->d_heads.as<int32_t>(), M->d_uid.as<int32_t>(), (size_t)ne, rocprim::plus<int32_t>(), st);
  };
  size_t sort_bytes = 0, scan_bytes = 0, flag_bytes = 0;
  VGX_HIP(ctx, temp_bytes(sort, &sort_bytes));
  VGX_HIP(ctx, temp_bytes(scan, &scan_bytes));
  VGX_HIP(ctx, temp_bytes(flag_scan, &flag_bytes));
  int rc = ensure_blocks(M, ne, std::max<size_t>(std::max(std::max(sort_bytes, scan_bytes), flag_bytes), 4));
  if (rc == VGX_OK) rc = ensure_entries(M, ne, n);
  if (rc != VGX_OK) return rc;
  // 1. descriptors, keys, one sort
  VGX_HIP(ctx, hipMemcpyAsync(M->d_src.p, M->h_src.data(), M->h_src.size() * sizeof(SepSrc), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(sep_keys_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, M->d_src.as<SepSrc>(), n, (int64_t)ne, box,
                     M->d_keys[0].as<unsigned long long>(), M->d_slots[0].as<int32_t>());
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, sort(M->d_tmp.p, sort_bytes));
  // 2. count, 3. scan the counts and the block heads; the unique blocks and their first triangles
  VGX_HIP(ctx, vps == 16 ? launch_separated<16>(false, st, ne, M, (unsigned long long)n, mw)
                         : launch_separated<8>(false, st, ne, M, (unsigned long long)n, mw));
  VGX_HIP(ctx, hipMemsetAsync(M->d_efirst.p, 0, sizeof(int64_t), st));
  VGX_HIP(ctx, scan(M->d_tmp.p, scan_bytes));
  VGX_HIP(ctx, flag_scan(M->d_tmp.p, flag_bytes));
  hipLaunchKernelGGL(sep_unique_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, M->d_src.as<SepSrc>(), (unsigned long long)n,
                     M->d_keys[1].as<unsigned long long>(), M->d_slots[1].as<int32_t>(), ne, M->d_heads.as<int32_t>(),
                     M->d_uid.as<int32_t>(), M->d_efirst.as<int64_t>(), M->d_block_index.as<int32_t>(), M->d_first.as<int64_t>(),
                     M->d_tail.as<int64_t>());
  VGX_HIP(ctx, hipGetLastError());
  int64_t tail[2] = {0, 0};
  VGX_HIP(ctx, hipMemcpyAsync(tail, M->d_tail.p, sizeof(tail), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  // 4. emit
  const int64_t total = tail[0];
  rc = ensure_tris(M, total);
  if (rc == VGX_OK) rc = ensure_colors(M, total);
  if (rc != VGX_OK) return rc;
  if (total > 0) {
    VGX_HIP(ctx, vps == 16 ? launch_separated<16>(true, st, ne, M, (unsigned long long)n, mw)
                           : launch_separated<8>(true, st, ne, M, (unsigned long long)n, mw));
    VGX_HIP(ctx, hipStreamSynchronize(st));
  }
  M->n_blocks = (int32_t)tail[1];
  M->n_tris = total;
  return VGX_OK;
}

// a finished submap's raw TSDF layer as a source
MeshSrc mesh_src(vgx_submap sm) {
  MeshSrc s{};
  s.lut = sm->d_lut;
  for (int a = 0; a < 3; ++a) {
    s.lut_min[a] = sm->lut_min[a];
    s.lut_dim[a] = sm->lut_dim[a];
  }
  s.block_index = sm->d_block_index;
  s.dist = sm->d_tsdf_distance;
  s.weight = sm->d_tsdf_weight;
  s.voxel_size = sm->voxel_size;
  return s;
}

// shared refusals; *mw the threshold to use
int check_args(vgx_ctx ctx, const vgx_mesh_config* cfg, vgx_mesh M, const char* fn, float* mw) {
  vgx_mesh_config c;
  vgx_mesh_config_default(&c);
  if (cfg) c = *cfg;
  if (!M) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL mesh");
  if (M->ctx != ctx) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": mesh of another context");
  if (!std::isfinite(c.min_weight) || c.min_weight < 0.0f)
    return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": min_weight negative or not finite");
  *mw = c.min_weight;
  return VGX_OK;
}

}  // namespace

namespace vgx {

std::mutex& mesh_mutex(vgx_mesh M) { return M->mu; }

MeshView mesh_view(vgx_mesh M) {
  MeshView v{};
  v.ctx = M->ctx;
  v.holds_mesh = M->holds_mesh;
  v.n_tris = M->n_tris;
  v.vertices = M->d_vertices.as<float>();
  v.normals = M->d_normals.as<float>();
  v.colors = M->has_colors ? M->d_colors.as<uint32_t>() : nullptr;
  v.has_colors = M->has_colors;
  v.per_vertex = M->per_vertex;
  return v;
}

}  // namespace vgx

extern "C" {

void vgx_mesh_config_default(vgx_mesh_config* cfg) {
  if (cfg) cfg->min_weight = 1e-4f;
}

int vgx_mesh_create(vgx_ctx ctx, vgx_mesh* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_mesh_create: NULL argument");
  vgx_mesh M = new vgx_mesh_s;
  M->ctx = ctx;
  *out = M;
  return VGX_OK;
}

int vgx_mesh_destroy(vgx_mesh M) {
  if (!M) return VGX_ERR_INVALID;
  (void)hipSetDevice(M->ctx->device);
  delete M;
  return VGX_OK;
}

}  // extern "C"

namespace {

// vgx_tsdf_layer_generate_mesh, and with colored the same passes plus the vertex-colour kernel (fn: the call's name)
int layer_generate_mesh(vgx_tsdf_layer L, const vgx_mesh_config* cfg, vgx_mesh M, bool colored, const char* fn) {
  if (!L) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(fn) + ": NULL layer");
  vgx_ctx ctx = L->ctx;
  float mw = 0.0f;
  int rc = check_args(ctx, cfg, M, fn, &mw);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> mesh_lk(M->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);  // (lock order: tsdf_mu, then mu -- as vgx_tsdf_layer_merge_submaps)
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  M->reset_stats();
  int32_t nb = 0;
  unsigned long long dropped = 0;
  rc = tsdf_read_stats(L, &nb, &dropped);  // (behind the scans and merges queued on the TSDF stream)
  if (rc != VGX_OK) return rc;
  const TsdfLayerDev& d = L->dev;
  MeshSrc s{};
  s.lut = d.lut;
  for (int a = 0; a < 3; ++a) {
    s.lut_min[a] = d.lut_min[a];
    s.lut_dim[a] = d.lut_dim[a];
  }
  s.block_index = d.block_index;
  s.words = d.voxels;
  s.voxel_size = d.voxel_size;
  rc = generate<true>(ctx, ctx->tsdf_stream, s, d.vps, nb, mw, M, colored ? d.rgba : nullptr);
  M->holds_mesh = rc == VGX_OK;
  M->has_colors = M->per_vertex = colored && rc == VGX_OK;
  return rc;
}

int submap_generate_mesh(vgx_submap sm, const vgx_mesh_config* cfg, vgx_mesh M, bool colored, const char* fn) {
  if (!sm) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(fn) + ": NULL submap");
  vgx_ctx ctx = sm->ctx;
  float mw = 0.0f;
  int rc = check_args(ctx, cfg, M, fn, &mw);
  if (rc != VGX_OK) return rc;
  if (sm->n_blocks > 0 && (!sm->d_tsdf_distance || !sm->d_tsdf_weight))
    return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": raw TSDF layer not resident (released?)");
  if (sm->vps != 8 && sm->vps != 16)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": voxels_per_side must be 8 or 16");
  std::lock_guard<std::mutex> mesh_lk(M->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  if (colored && !sm->d_tsdf_rgba) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": the submap has no colours");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  M->reset_stats();
  rc = generate<false>(ctx, ctx->stream, mesh_src(sm), sm->vps, sm->n_blocks, mw, M, colored ? sm->d_tsdf_rgba : nullptr);
  M->holds_mesh = rc == VGX_OK;
  M->has_colors = M->per_vertex = colored && rc == VGX_OK;
  return rc;
}

}  // namespace

extern "C" {

int vgx_tsdf_layer_generate_mesh(vgx_tsdf_layer L, const vgx_mesh_config* cfg, vgx_mesh M) {
  return layer_generate_mesh(L, cfg, M, false, "vgx_tsdf_layer_generate_mesh");
}

int vgx_tsdf_layer_generate_mesh_colored(vgx_tsdf_layer L, const vgx_mesh_config* cfg, vgx_mesh M) {
  return layer_generate_mesh(L, cfg, M, true, "vgx_tsdf_layer_generate_mesh_colored");
}

int vgx_submap_generate_mesh(vgx_submap sm, const vgx_mesh_config* cfg, vgx_mesh M) {
  return submap_generate_mesh(sm, cfg, M, false, "vgx_submap_generate_mesh");
}

int vgx_submap_generate_mesh_colored(vgx_submap sm, const vgx_mesh_config* cfg, vgx_mesh M) {
  return submap_generate_mesh(sm, cfg, M, true, "vgx_submap_generate_mesh_colored");
}

int vgx_submaps_generate_separated_mesh(vgx_ctx ctx, int32_t n, const vgx_submap* submaps, const float* T_M_S, const uint8_t* rgba,
                                        const vgx_mesh_config* cfg, vgx_mesh M) {
  static const char* kFn = "vgx_submaps_generate_separated_mesh: ";
  auto fail = [ctx](int code, const std::string& msg) { return set_error(ctx, code, kFn + msg); };
  if (!ctx) return set_error(nullptr, VGX_ERR_INVALID, std::string(kFn) + "NULL context");
  float mw = 0.0f;
  int rc = check_args(ctx, cfg, M, "vgx_submaps_generate_separated_mesh", &mw);
  if (rc != VGX_OK) return rc;
  if (n < 0) return fail(VGX_ERR_INVALID, "n < 0");
  if (n > 0 && (!submaps || !T_M_S || !rgba)) return fail(VGX_ERR_INVALID, "NULL submaps / T_M_S / rgba with n > 0");
  int64_t n_entries = 0;
  long long lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
  bool any = false;
  for (int32_t i = 0; i < n; ++i) {
    const vgx_submap sm = submaps[i];
    const std::string at = "submap " + std::to_string(i) + ": ";
    if (!sm || sm->ctx != ctx) return fail(VGX_ERR_INVALID, at + "NULL or of another context");
    if (sm->n_blocks > 0 && (!sm->d_tsdf_distance || !sm->d_tsdf_weight))
      return fail(VGX_ERR_INVALID, at + "raw TSDF layer not resident (released?)");
    if (sm->voxel_size != submaps[0]->voxel_size || sm->vps != submaps[0]->vps)
      return fail(VGX_ERR_INVALID, at + "voxel_size / voxels_per_side differ from submap 0's");
    const PoseDefect bad = pose_defect(T_M_S + 7 * (size_t)i);
    if (bad == kPoseNotFinite) return fail(VGX_ERR_INVALID, at + "pose value not finite");
    if (bad == kPoseNotUnit) return fail(VGX_ERR_INVALID, at + "pose quaternion not unit (|q|^2 - 1 > 1e-4)");
    n_entries += sm->n_blocks;
    if (sm->n_blocks == 0) continue;
    for (int a = 0; a < 3; ++a) {
      const long long l = sm->lut_min[a], h = (long long)sm->lut_min[a] + sm->lut_dim[a] - 1;
      lo[a] = any ? std::min(lo[a], l) : l;
      hi[a] = any ? std::max(hi[a], h) : h;
    }
    any = true;
  }
  if (n > 0 && submaps[0]->vps != 8 && submaps[0]->vps != 16) return fail(VGX_ERR_UNSUPPORTED, "voxels_per_side must be 8 or 16");
  if (n_entries > INT32_MAX) return fail(VGX_ERR_UNSUPPORTED, "more than 2^31 - 1 blocks in all");
  SepBox box{};
  unsigned end_bit = 1;
  if (any) {
    unsigned __int128 cells = 1;
    for (int a = 0; a < 3; ++a) {
      box.lo[a] = lo[a];
      box.dim[a] = (unsigned long long)(hi[a] - lo[a] + 1);
      cells *= box.dim[a];
    }
    const unsigned __int128 keys = cells * (unsigned __int128)n;  // (dims < 2^33 each: no overflow of 128 bits)
    if (keys > ((unsigned __int128)1 << 64)) return fail(VGX_ERR_UNSUPPORTED, "union block box x n does not fit a 64-bit key");
    while (end_bit < 64 && ((unsigned __int128)1 << end_bit) < keys) ++end_bit;
  }
  std::lock_guard<std::mutex> mesh_lk(M->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  M->reset_stats();
  if (n_entries == 0) {
    M->has_colors = true;
    M->holds_mesh = true;
    return VGX_OK;
  }
  M->h_src.assign((size_t)n, SepSrc{});
  int64_t e0 = 0;
  for (int32_t i = 0; i < n; ++i) {
    const vgx_submap sm = submaps[i];
    SepSrc& d = M->h_src[(size_t)i];
    d.m = mesh_src(sm);
    const float* T = T_M_S + 7 * (size_t)i;
    for (int k = 0; k < 4; ++k) d.pose.q[k] = T[k];
    for (int k = 0; k < 3; ++k) d.pose.t[k] = T[4 + k];
    std::memcpy(&d.pose.rgba, rgba + 4 * (size_t)i, 4);
    d.entry0 = e0;
    e0 += sm->n_blocks;
  }
  rc = generate_separated(ctx, ctx->stream, submaps[0]->vps, (int32_t)n_entries, box, end_bit, mw, M);
  if (rc != VGX_OK) {
    M->n_blocks = 0;
    M->n_tris = 0;
    return rc;
  }
  M->has_colors = true;
  M->holds_mesh = true;
  return VGX_OK;
}

int vgx_mesh_has_colors(vgx_mesh M, int32_t* has) {
  if (!M || !has) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, "vgx_mesh_has_colors: NULL argument");
  std::lock_guard<std::mutex> lk(M->mu);
  *has = M->has_colors ? 1 : 0;
  return VGX_OK;
}

int vgx_mesh_color_layout(vgx_mesh M, int32_t* layout) {
  if (!M || !layout) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, "vgx_mesh_color_layout: NULL argument");
  std::lock_guard<std::mutex> lk(M->mu);
  *layout = !M->has_colors ? VGX_MESH_COLORS_NONE : (M->per_vertex ? VGX_MESH_COLORS_PER_VERTEX : VGX_MESH_COLORS_PER_TRIANGLE);
  return VGX_OK;
}

int vgx_mesh_download_colors(vgx_mesh M, uint8_t* rgba) {
  if (!M || !rgba) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, "vgx_mesh_download_colors: NULL argument");
  vgx_ctx ctx = M->ctx;
  std::lock_guard<std::mutex> lk(M->mu);
  if (!M->has_colors) return set_error(ctx, VGX_ERR_INVALID, "vgx_mesh_download_colors: the mesh has no colours");
  if (M->per_vertex)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_mesh_download_colors: one colour per vertex (vgx_mesh_download_vertex_colors)");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  if (M->n_tris > 0) VGX_HIP(ctx, hipMemcpy(rgba, M->d_colors.p, (size_t)M->n_tris * 4, hipMemcpyDeviceToHost));
  return VGX_OK;
}

int vgx_mesh_download_vertex_colors(vgx_mesh M, uint8_t* rgba) {
  if (!M || !rgba) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, "vgx_mesh_download_vertex_colors: NULL argument");
  vgx_ctx ctx = M->ctx;
  std::lock_guard<std::mutex> lk(M->mu);
  if (!M->has_colors || !M->per_vertex)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_mesh_download_vertex_colors: the mesh has no per-vertex colours");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  if (M->n_tris > 0) VGX_HIP(ctx, hipMemcpy(rgba, M->d_colors.p, (size_t)M->n_tris * 12, hipMemcpyDeviceToHost));
  return VGX_OK;
}

int vgx_mesh_stats(vgx_mesh M, int32_t* n_blocks, int64_t* n_triangles) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  if (n_blocks) *n_blocks = M->n_blocks;
  if (n_triangles) *n_triangles = M->n_tris;
  return VGX_OK;
}

int vgx_mesh_download(vgx_mesh M, int32_t* block_index, int64_t* first, float* vertices, float* normals) {
  if (!M) return VGX_ERR_INVALID;
  vgx_ctx ctx = M->ctx;
  std::lock_guard<std::mutex> lk(M->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t nb = M->n_blocks, nt = M->n_tris;
  if (first && nb == 0) first[0] = 0;
  if (nb > 0) {
    if (block_index) VGX_HIP(ctx, hipMemcpy(block_index, M->d_block_index.p, (size_t)nb * 12, hipMemcpyDeviceToHost));
    if (first) VGX_HIP(ctx, hipMemcpy(first, M->d_first.p, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost));
  }
  if (nt > 0) {
    if (vertices) VGX_HIP(ctx, hipMemcpy(vertices, M->d_vertices.p, (size_t)nt * 36, hipMemcpyDeviceToHost));
    if (normals) VGX_HIP(ctx, hipMemcpy(normals, M->d_normals.p, (size_t)nt * 12, hipMemcpyDeviceToHost));
  }
  return VGX_OK;
}

int vgx_mesh_triangle_table(int8_t out[256][16]) {
  if (!out) return VGX_ERR_INVALID;
  std::memcpy(out, kMcTriangleTable, sizeof(kMcTriangleTable));
  return VGX_OK;
}

int vgx_mesh_write_ply(vgx_mesh M, const char* path) {
  if (!M || !path) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, "vgx_mesh_write_ply: NULL argument");
  int64_t nt = 0;
  int rc = vgx_mesh_stats(M, nullptr, &nt);
  if (rc != VGX_OK) return rc;
  if (3 * nt > INT32_MAX) return set_error(M->ctx, VGX_ERR_UNSUPPORTED, "vgx_mesh_write_ply: more than 2^31 vertices (int indices)");
  std::vector<float> v((size_t)nt * 9), n((size_t)nt * 3);
  rc = vgx_mesh_download(M, nullptr, nullptr, v.data(), n.data());
  if (rc != VGX_OK) return rc;
  int32_t colored = 0;  // VGX_MESH_COLORS_*
  std::vector<uint8_t> rgba;
  rc = vgx_mesh_color_layout(M, &colored);
  const size_t cstride = colored == VGX_MESH_COLORS_PER_VERTEX ? 4 : 0;  // bytes from one corner's colour to the next
  if (rc == VGX_OK && colored == VGX_MESH_COLORS_PER_VERTEX) {
    rgba.resize((size_t)nt * 12);
    rc = vgx_mesh_download_vertex_colors(M, rgba.data());
  } else if (rc == VGX_OK && colored) {
    rgba.resize((size_t)nt * 4);
    rc = vgx_mesh_download_colors(M, rgba.data());
  }
  if (rc != VGX_OK) return rc;
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return set_error(M->ctx, VGX_ERR_INVALID, std::string("vgx_mesh_write_ply: cannot open ") + path);
  const std::string header = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(3 * nt) +
                             "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
                             "property float nz\n" +
                             (colored ? "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n" : "") +
                             "element face " + std::to_string(nt) +
                             "\nproperty list uchar int vertex_indices\nend_header\n";
  bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size();
  std::vector<float> vrec;
  std::vector<unsigned char> frec;
  constexpr int64_t kChunk = 1 << 16;  // triangles per write
  for (int64_t t0 = 0; ok && colored && t0 < nt; t0 += kChunk) {  // x y z nx ny nz (f32) r g b a (u8): 28 B per vertex
    const int64_t t1 = std::min(nt, t0 + kChunk);
    frec.assign((size_t)(t1 - t0) * 3 * 28, 0);
    for (int64_t t = t0; t < t1; ++t)
      for (int q = 0; q < 3; ++q) {
        unsigned char* r = &frec[((size_t)(t - t0) * 3 + q) * 28];
        std::memcpy(r, &v[(size_t)t * 9 + 3 * q], 12);
        std::memcpy(r + 12, &n[(size_t)t * 3], 12);
        std::memcpy(r + 24, &rgba[(size_t)t * (4 + 2 * cstride) + q * cstride], 4);
      }
    ok = std::fwrite(frec.data(), 1, frec.size(), f) == frec.size();
  }
  for (int64_t t0 = 0; ok && !colored && t0 < nt; t0 += kChunk) {
    const int64_t t1 = std::min(nt, t0 + kChunk);
    vrec.clear();
    for (int64_t t = t0; t < t1; ++t)
      for (int q = 0; q < 3; ++q) {
        vrec.insert(vrec.end(), &v[(size_t)t * 9 + 3 * q], &v[(size_t)t * 9 + 3 * q] + 3);
        vrec.insert(vrec.end(), &n[(size_t)t * 3], &n[(size_t)t * 3] + 3);
      }
    ok = std::fwrite(vrec.data(), sizeof(float), vrec.size(), f) == vrec.size();
  }
  for (int64_t t0 = 0; ok && t0 < nt; t0 += kChunk) {
    const int64_t t1 = std::min(nt, t0 + kChunk);
    frec.assign((size_t)(t1 - t0) * 13, 0);
    for (int64_t t = t0; t < t1; ++t) {
      unsigned char* r = &frec[(size_t)(t - t0) * 13];
      r[0] = 3;
      for (int q = 0; q < 3; ++q) {
        const int32_t idx = (int32_t)(3 * t + q);
        std::memcpy(r + 1 + 4 * q, &idx, 4);
      }
    }
    ok = std::fwrite(frec.data(), 1, frec.size(), f) == frec.size();
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) return set_error(M->ctx, VGX_ERR_INVALID, std::string("vgx_mesh_write_ply: write failed: ") + path);
  return VGX_OK;
}

}  // extern "C"
