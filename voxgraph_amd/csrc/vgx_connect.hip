// The connected mesh on the device: voxblox MeshLayer::getConnectedMesh / createConnectedMesh [recalled] over the triangle
// soup a vgx_mesh holds.  The rules are stated in include/voxgraph_amd.h (vgx_mesh_connect); the layout and the passes in
// DESIGN.md 15.
//
//   1. insert   one thread per soup vertex j: its 192-bit key (three int64 cells), a probe of a power-of-two table of u32
//               slots (>= 2 x 3T, empty = 0xFFFFFFFF).  An empty slot is claimed by atomicCAS(empty -> j).  An occupied
//               slot names a vertex; its key is recomputed from the soup (12 bytes) and compared exactly: equal ->
//               atomicMin(slot, j) when j is smaller, else the next slot.  A slot's key never changes (only which of its
//               vertices represents it) and slots are never freed, so a key always ends in the same slot.
//   2. resolve  one thread per j probes again and reads the slot's final value rep[j]; flag[j] = (rep[j] == j)
//   3. scan     an inclusive scan of the flags: a representative's number is scan[j] - 1, V = scan[3T - 1]; V and the
//               out-of-range flag come back in one synchronisation; the output arrays grow once
//   4. emit     representatives copy vertex, normal and colour to their number; every j writes indices[j]
// The only atomics are the claim, the minimum and the out-of-range flag's OR: integers whose final value does not depend
// on the order of arrival, so values and order do not depend on scheduling.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "vgx_internal.h"

#include <rocprim/rocprim.hpp>

#pragma clang fp contract(off)

namespace vgx {

constexpr uint32_t kConnectEmpty = 0xFFFFFFFFu;
constexpr int kConnectThreads = 256;

struct ConnectKey {
  long long k[3];
};

// k = (int64) round((double)v * inv) per coordinate; false when a coordinate is not finite or |v * inv| >= 2^62
__device__ __forceinline__ bool connect_key(const float* __restrict__ v, double inv, ConnectKey& key) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double p = (double)v[a] * inv;
    const bool in = fabs(p) < 0x1p62;  // (false for NaN and the infinities)
    key.k[a] = in ? (long long)round(p) : 0;  // round: halves away from zero; -0.0 -> 0
    ok = ok && in;
  }
  return ok;
}

__device__ __forceinline__ bool connect_equal(const ConnectKey& a, const ConnectKey& b) {
  return a.k[0] == b.k[0] && a.k[1] == b.k[1] && a.k[2] == b.k[2];
}

__device__ __forceinline__ unsigned long long connect_mix(unsigned long long x) {  // splitmix64's finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// finds the slot, never decides equality
__device__ __forceinline__ unsigned long long connect_hash(const ConnectKey& key) {
  unsigned long long h = connect_mix((unsigned long long)key.k[0] + 0x9e3779b97f4a7c15ull);
  h = connect_mix(h ^ (unsigned long long)key.k[1]);
  return connect_mix(h ^ (unsigned long long)key.k[2]);
}

__global__ __launch_bounds__(kConnectThreads) void connect_insert_kernel(const float* __restrict__ soup, uint32_t n, double inv,
                                                                         uint32_t* __restrict__ table, unsigned long long mask,
                                                                         int32_t* __restrict__ bad) {
  const unsigned long long g = (unsigned long long)blockIdx.x * kConnectThreads + threadIdx.x;
  if (g >= n) return;
  const uint32_t j = (uint32_t)g;
  ConnectKey key;
  if (!connect_key(soup + 3 * (size_t)j, inv, key)) {
    atomicOr(bad, 1);
    return;
  }
  unsigned long long h = connect_hash(key) & mask;
  while (true) {  // (the table holds >= 2 n slots: an empty one is always met)
    // a stale value is harmless: it is `empty` (the claim below then returns the truth) or an earlier representative of
    // the slot's one key (the comparison gives the same answer, the minimum is taken by the atomic)
    uint32_t cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kConnectEmpty) {
      cur = atomicCAS(&table[h], kConnectEmpty, j);
      if (cur == kConnectEmpty) return;
    }
    ConnectKey other;
    connect_key(soup + 3 * (size_t)cur, inv, other);  // (cur is in the table: it passed the range check)
    if (connect_equal(key, other)) {
      if (j < cur) atomicMin(&table[h], j);
      return;
    }
    h = (h + 1) & mask;
  }
}

__global__ __launch_bounds__(kConnectThreads) void connect_resolve_kernel(const float* __restrict__ soup, uint32_t n, double inv,
                                                                          const uint32_t* __restrict__ table, unsigned long long mask,
                                                                          uint32_t* __restrict__ rep, uint32_t* __restrict__ flag) {
  const unsigned long long g = (unsigned long long)blockIdx.x * kConnectThreads + threadIdx.x;
  if (g >= n) return;
  const uint32_t j = (uint32_t)g;
  ConnectKey key;
  uint32_t r = j;  // (an out-of-range vertex was not inserted: the call fails, nothing reads this)
  if (connect_key(soup + 3 * (size_t)j, inv, key)) {
    unsigned long long h = connect_hash(key) & mask;
    while (true) {
      const uint32_t cur = table[h];
      if (cur == j || cur == kConnectEmpty) break;  // (empty: not reached, every key was inserted)
      ConnectKey other;
      connect_key(soup + 3 * (size_t)cur, inv, other);
      if (connect_equal(key, other)) {
        r = cur;
        break;
      }
      h = (h + 1) & mask;
    }
  }
  rep[j] = r;
  flag[j] = r == j ? 1u : 0u;
}

// number [n]: the inclusive scan of the flags
__global__ __launch_bounds__(kConnectThreads) void connect_emit_kernel(const float* __restrict__ soup, const float* __restrict__ tri_normals,
                                                                       const uint32_t* __restrict__ tri_colors, bool per_vertex, uint32_t n,
                                                                       const uint32_t* __restrict__ rep, const uint32_t* __restrict__ number,
                                                                       float* __restrict__ vertices, float* __restrict__ normals,
                                                                       uint32_t* __restrict__ colors, uint32_t* __restrict__ indices) {
  const unsigned long long g = (unsigned long long)blockIdx.x * kConnectThreads + threadIdx.x;
  if (g >= n) return;
  const uint32_t j = (uint32_t)g;
  const uint32_t r = rep[j];
  const uint32_t u = number[r] - 1u;
  indices[j] = u;
  if (r != j) return;
  const size_t t = j / 3u;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    vertices[3 * (size_t)u + a] = soup[3 * (size_t)j + a];
    normals[3 * (size_t)u + a] = tri_normals[3 * t + a];
  }
  if (tri_colors) colors[u] = tri_colors[per_vertex ? (size_t)j : t];  // (per vertex: the first soup vertex's own colour)
}

}  // namespace vgx

using namespace vgx;

struct vgx_connected_mesh_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  int64_t n_verts = 0, n_tris = 0;  // the mesh held now
  bool has_colors = false;
  // output, grown on demand
  DeviceBuffer d_vertices;  // float [vert_cap][3]
  DeviceBuffer d_normals;   // float [vert_cap][3]
  DeviceBuffer d_colors;    // u32 [vert_cap] bytes r g b a
  DeviceBuffer d_indices;   // u32 [soup_cap]: [T][3]
  // scratch
  DeviceBuffer d_table;     // u32 [table_slots(soup_cap)] slots
  DeviceBuffer d_rep;       // u32 [soup_cap]
  DeviceBuffer d_number;    // u32 [soup_cap]: flags, then their inclusive scan
  DeviceBuffer d_bad;       // int32: the out-of-range flag
  DeviceBuffer d_tmp;       // the scan's workspace
};

namespace {

// the power of two >= 2 n (n < 2^32)
int64_t table_slots(int64_t n) {
  int64_t s = 1024;
  while (s < 2 * n) s <<= 1;
  return s;
}

// a quarter of slack (the next map is a little larger), at least 4096 vertices
size_t vertex_capacity(int64_t n) { return (size_t)std::max<int64_t>(n + n / 4, 4096); }

// per-soup-vertex arrays (indices, rep, number), the table (sized from the capacity) and the scan's workspace, which goes
// when they go
int ensure_soup(vgx_connected_mesh C, int64_t n, size_t tmp_bytes) {
  if ((size_t)n * 4 > C->d_rep.bytes) {
    const size_t cap = vertex_capacity(n);
    C->d_tmp.release();
    const hipError_t e = alloc_group({{&C->d_indices, cap * 4}, {&C->d_rep, cap * 4}, {&C->d_number, cap * 4},
                                      {&C->d_table, (size_t)table_slots((int64_t)cap) * 4}, {&C->d_bad, sizeof(int32_t)}});
    if (e != hipSuccess) return alloc_error(C->ctx, e, "connected mesh: allocating per-vertex arrays and table");
  }
  const hipError_t e = C->d_tmp.reserve(tmp_bytes);
  return e == hipSuccess ? VGX_OK : alloc_error(C->ctx, e, "connected mesh: allocating scan workspace");
}

int ensure_verts(vgx_connected_mesh C, int64_t nv) {
  if ((size_t)nv * 4 <= C->d_colors.bytes) return VGX_OK;
  const size_t cap = vertex_capacity(nv);
  const hipError_t e = alloc_group({{&C->d_vertices, cap * 12}, {&C->d_normals, cap * 12}, {&C->d_colors, cap * 4}});
  return e == hipSuccess ? VGX_OK : alloc_error(C->ctx, e, "connected mesh: allocating vertices");
}

// the passes over n = 3 T > 0 soup vertices, on `st` (the caller holds both handles' locks and the registration lock,
// and has reset C's stats)
int connect(vgx_ctx ctx, hipStream_t st, const MeshView& src, double inv, vgx_connected_mesh C) {
  const int64_t n = 3 * src.n_tris;
  // all the room is made before the first launch
  auto scan = [&](void* tmp, size_t& bytes) {
    return rocprim::inclusive_scan(tmp, bytes, C->d_number.as<uint32_t>(), C->d_number.as<uint32_t>(), (size_t)n,
                                   rocprim::plus<uint32_t>(), st);
  };
  size_t scan_bytes = 0;
  VGX_HIP(ctx, temp_bytes(scan, &scan_bytes));
  int rc = ensure_soup(C, n, std::max<size_t>(scan_bytes, 4));
  if (rc != VGX_OK) return rc;
  const int64_t slots = table_slots(n);  // (<= the table's capacity: table_slots is monotone)
  uint32_t* const table = C->d_table.as<uint32_t>();
  uint32_t* const rep = C->d_rep.as<uint32_t>();
  uint32_t* const number = C->d_number.as<uint32_t>();
  int32_t* const d_bad = C->d_bad.as<int32_t>();
  const unsigned long long mask = (unsigned long long)slots - 1ull;
  const dim3 grid((unsigned)((n + kConnectThreads - 1) / kConnectThreads)), block(kConnectThreads);
  const uint32_t n32 = (uint32_t)n;
  // 1. insert
  VGX_HIP(ctx, hipMemsetAsync(table, 0xFF, (size_t)slots * 4, st));
  VGX_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(connect_insert_kernel, grid, block, 0, st, src.vertices, n32, inv, table, mask, d_bad);
  VGX_HIP(ctx, hipGetLastError());
  // 2. resolve, 3. scan
  hipLaunchKernelGGL(connect_resolve_kernel, grid, block, 0, st, src.vertices, n32, inv, table, mask, rep, number);
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, scan(C->d_tmp.p, scan_bytes));
  uint32_t nv = 0;
  int32_t bad = 0;
  VGX_HIP(ctx, hipMemcpyAsync(&nv, number + (n - 1), sizeof(nv), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  if (bad)
    return set_error(ctx, VGX_ERR_UNSUPPORTED,
                     "vgx_mesh_connect: a vertex coordinate is not finite or |v / threshold| >= 2^62 (no int64 cell)");
  // 4. emit
  rc = ensure_verts(C, nv);
  if (rc != VGX_OK) return rc;
  hipLaunchKernelGGL(connect_emit_kernel, grid, block, 0, st, src.vertices, src.normals, src.colors, src.per_vertex, n32, rep, number,
                     C->d_vertices.as<float>(), C->d_normals.as<float>(), C->d_colors.as<uint32_t>(), C->d_indices.as<uint32_t>());
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, hipStreamSynchronize(st));
  C->n_verts = nv;
  C->n_tris = src.n_tris;
  return VGX_OK;
}

}  // namespace

extern "C" {

int vgx_connected_mesh_create(vgx_ctx ctx, vgx_connected_mesh* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_connected_mesh_create: NULL argument");
  vgx_connected_mesh C = new vgx_connected_mesh_s;
  C->ctx = ctx;
  *out = C;
  return VGX_OK;
}

int vgx_connected_mesh_destroy(vgx_connected_mesh C) {
  if (!C) return VGX_ERR_INVALID;
  (void)hipSetDevice(C->ctx->device);
  delete C;
  return VGX_OK;
}

int vgx_mesh_connect(vgx_mesh M, float threshold, vgx_connected_mesh C) {
  static const char* kFn = "vgx_mesh_connect: ";
  if (!M) return set_error(C ? C->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + "NULL mesh");
  vgx_ctx ctx = mesh_view(M).ctx;
  if (!C) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "NULL connected mesh");
  if (C->ctx != ctx) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "connected mesh of another context");
  if (!std::isfinite(threshold) || !(threshold > 0.0f))
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "threshold not finite or not > 0");
  std::lock_guard<std::mutex> out_lk(C->mu);
  std::lock_guard<std::mutex> mesh_lk(mesh_mutex(M));
  const MeshView src = mesh_view(M);
  if (!src.holds_mesh) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "the source handle holds no mesh (its last call failed)");
  if (3 * src.n_tris >= ((int64_t)1 << 32)) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + "3 T >= 2^32 (u32 indices)");
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  C->n_verts = 0;
  C->n_tris = 0;
  C->has_colors = src.has_colors;
  if (src.n_tris == 0) return VGX_OK;
  const double inv = 1.0 / (double)threshold;
  const int rc = connect(ctx, ctx->stream, src, inv, C);
  if (rc != VGX_OK) C->has_colors = false;  // (the handle holds no mesh: stats report 0)
  return rc;
}

int vgx_connected_mesh_stats(vgx_connected_mesh C, int64_t* n_vertices, int64_t* n_triangles, int32_t* has_colors) {
  if (!C) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(C->mu);
  if (n_vertices) *n_vertices = C->n_verts;
  if (n_triangles) *n_triangles = C->n_tris;
  if (has_colors) *has_colors = C->has_colors ? 1 : 0;
  return VGX_OK;
}

int vgx_connected_mesh_download(vgx_connected_mesh C, float* vertices, float* normals, uint8_t* rgba, uint32_t* indices) {
  if (!C) return VGX_ERR_INVALID;
  vgx_ctx ctx = C->ctx;
  std::lock_guard<std::mutex> lk(C->mu);
  if (rgba && !C->has_colors) return set_error(ctx, VGX_ERR_INVALID, "vgx_connected_mesh_download: the mesh has no colours");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t nv = C->n_verts, nt = C->n_tris;
  if (nv > 0) {
    if (vertices) VGX_HIP(ctx, hipMemcpy(vertices, C->d_vertices.p, (size_t)nv * 12, hipMemcpyDeviceToHost));
    if (normals) VGX_HIP(ctx, hipMemcpy(normals, C->d_normals.p, (size_t)nv * 12, hipMemcpyDeviceToHost));
    if (rgba) VGX_HIP(ctx, hipMemcpy(rgba, C->d_colors.p, (size_t)nv * 4, hipMemcpyDeviceToHost));
  }
  if (nt > 0 && indices) VGX_HIP(ctx, hipMemcpy(indices, C->d_indices.p, (size_t)nt * 12, hipMemcpyDeviceToHost));
  return VGX_OK;
}

int vgx_connected_mesh_write_ply(vgx_connected_mesh C, const char* path) {
  if (!C || !path) return set_error(C ? C->ctx : nullptr, VGX_ERR_INVALID, "vgx_connected_mesh_write_ply: NULL argument");
  int64_t nv = 0, nt = 0;
  int32_t colored = 0;
  int rc = vgx_connected_mesh_stats(C, &nv, &nt, &colored);
  if (rc != VGX_OK) return rc;
  if (nv > INT32_MAX) return set_error(C->ctx, VGX_ERR_UNSUPPORTED, "vgx_connected_mesh_write_ply: V >= 2^31 (int indices)");
  std::vector<float> v((size_t)nv * 3), n((size_t)nv * 3);
  std::vector<uint8_t> rgba(colored ? (size_t)nv * 4 : 0);
  std::vector<uint32_t> idx((size_t)nt * 3);
  rc = vgx_connected_mesh_download(C, v.data(), n.data(), colored ? rgba.data() : nullptr, idx.data());
  if (rc != VGX_OK) return rc;
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return set_error(C->ctx, VGX_ERR_INVALID, std::string("vgx_connected_mesh_write_ply: cannot open ") + path);
  const std::string header = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(nv) +
                             "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
                             "property float nz\n" +
                             (colored ? "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n" : "") +
                             "element face " + std::to_string(nt) + "\nproperty list uchar int vertex_indices\nend_header\n";
  bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size();
  std::vector<unsigned char> rec;
  constexpr int64_t kChunk = 1 << 16;  // records per write
  const size_t vsize = colored ? 28 : 24;
  for (int64_t i0 = 0; ok && i0 < nv; i0 += kChunk) {  // x y z nx ny nz (f32), then r g b a (u8)
    const int64_t i1 = std::min(nv, i0 + kChunk);
    rec.assign((size_t)(i1 - i0) * vsize, 0);
    for (int64_t i = i0; i < i1; ++i) {
      unsigned char* r = &rec[(size_t)(i - i0) * vsize];
      std::memcpy(r, &v[(size_t)i * 3], 12);
      std::memcpy(r + 12, &n[(size_t)i * 3], 12);
      if (colored) std::memcpy(r + 24, &rgba[(size_t)i * 4], 4);
    }
    ok = std::fwrite(rec.data(), 1, rec.size(), f) == rec.size();
  }
  for (int64_t t0 = 0; ok && t0 < nt; t0 += kChunk) {
    const int64_t t1 = std::min(nt, t0 + kChunk);
    rec.assign((size_t)(t1 - t0) * 13, 0);
    for (int64_t t = t0; t < t1; ++t) {
      unsigned char* r = &rec[(size_t)(t - t0) * 13];
      r[0] = 3;
      std::memcpy(r + 1, &idx[(size_t)t * 3], 12);  // (V < 2^31: the u32 are the int values)
    }
    ok = std::fwrite(rec.data(), 1, rec.size(), f) == rec.size();
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) return set_error(C->ctx, VGX_ERR_INVALID, std::string("vgx_connected_mesh_write_ply: write failed: ") + path);
  return VGX_OK;
}

}  // extern "C"
