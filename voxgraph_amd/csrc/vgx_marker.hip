// Mesh markers on the device: voxblox_ros fillMarkerWithMesh [recalled] over the triangle soup a vgx_mesh holds -- the
// marker.points (three f64 per vertex) and marker.colors (four f32 per vertex, shaded by voxblox's ColorMode) of the three
// visualization_msgs/Marker meshes voxgraph publishes (SubmapVisuals::publishMesh / publishSeparatedMesh /
// publishCombinedMesh, submap_visuals.cpp:45-87).  The rules are stated in include/voxgraph_amd.h ("Mesh markers"), the
// kernel's resources and the measurement in DESIGN.md 19.
//
//   marker_fill_kernel<MODE>   one workgroup of 256 threads per 256 consecutive triangles, three steps:
//     table    thread i copies c8[i] (the 256 f32 of (float)((double)k / 255.0), built on the host) into LDS
//     colour   thread i shades triangle 256 b + i ONCE (every mode but HEIGHT: one colour per triangle) into LDS
//     points   the workgroup's 2304 soup floats are one contiguous run: thread i widens the float pairs i, i + 256, ..
//              (8-byte loads) into 16-byte stores, so a wave's store covers 1024 contiguous bytes
//     colours  thread i writes the 16 bytes of vertices i, i + 256, i + 512 of the workgroup (the LDS colour of triangle
//              vertex / 3, or under HEIGHT the rainbow of the vertex's own z): again 1024 contiguous bytes per wave
// No atomics, no scan: T is known on the host, and every output byte has one writer.
// PV (COLOR and LAMBERT_COLOR on a mesh with one colour per soup vertex): the colour step keeps only the triangle's two
// light terms in LDS, and the colours step shades vertex j from its own word vert_colors[j] (a wave reads 256 contiguous
// bytes) through the same table and formulas; the stores are the same 1024 contiguous bytes per wave.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>

#include "vgx_internal.h"

#pragma clang fp contract(off)

namespace vgx {

constexpr int kMarkerThreads = 256;  // threads, and triangles, per workgroup

struct MarkerParams {
  float light1[3], light2[3];  // L1, L2 normalised on the host
  float opacity;
  uint32_t constant_rgba;      // bytes r g b a; read when the kernel gets no colour array
};

__device__ __forceinline__ float marker_lambert(float c, float d1, float d2) {
  const float v = (d1 * c + d2 * c) + 0.2f;
  return (1.0f < v) ? 1.0f : v;
}

__device__ __forceinline__ float marker_light(const float n[3], const float L[3]) {
  const float d = (n[0] * L[0] + n[1] * L[1]) + n[2] * L[2];
  return (d < 0.0f) ? 0.0f : d;
}

// voxblox rainbowColorMap(h) [recalled] for a height ratio t in [0, 1], its three truncated channel bytes through c8
__device__ __forceinline__ void marker_height(float z, const float* __restrict__ c8, float rgb[3]) {
  float t = (float)(((double)z + 1.0) / 11.0);
  t = (t < 0.0f) ? 0.0f : t;
  t = (1.0f < t) ? 1.0f : t;
  double h = (double)t;
  h -= floor(h);
  h *= 6.0;
  const int i = (t == t) ? (int)floor(h) : -1;  // (a z that is not a number: the default case below)
  double f = h - (double)i;
  if (!(i & 1)) f = 1.0 - f;
  const uint32_t hi = 255u, lo = 0u, mid = (uint32_t)(255.0 * (1.0 - f));  // (0 <= f <= 1: mid is 0 .. 255)
  uint32_t r = 255u, g = 127u, b = 127u;  // rainbowColorMap's default case
  switch (i) {
    case 6:
    case 0: r = hi; g = mid; b = lo; break;
    case 1: r = mid; g = hi; b = lo; break;
    case 2: r = lo; g = hi; b = mid; break;
    case 3: r = lo; g = mid; b = hi; break;
    case 4: r = mid; g = lo; b = hi; break;
    case 5: r = hi; g = lo; b = mid; break;
    default: break;
  }
  rgb[0] = c8[r & 255u];
  rgb[1] = c8[g & 255u];
  rgb[2] = c8[b & 255u];
}

// soup [T][3][3], tri_normals [T][3], tri_colors [T] (bytes r g b a) or null: P.constant_rgba for every triangle.
// points [3 T][3] f64 and colors [3 T][4] f32 are 16-byte aligned (device allocations).
template <int MODE, bool PV = false>
__global__ __launch_bounds__(kMarkerThreads) void marker_fill_kernel(const float* __restrict__ soup, const float* __restrict__ tri_normals,
                                                                     const uint32_t* __restrict__ tri_colors, unsigned long long n_tris,
                                                                     const float* __restrict__ c8, MarkerParams P,
                                                                     double* __restrict__ points, float4* __restrict__ colors) {
  __shared__ float s_c8[256];
  __shared__ float4 s_colour[kMarkerThreads];
  const unsigned i = threadIdx.x;
  const unsigned long long b = blockIdx.x;
  constexpr bool kTable = MODE == VGX_MARKER_COLOR || MODE == VGX_MARKER_LAMBERT_COLOR || MODE == VGX_MARKER_HEIGHT;
  if (kTable) s_c8[i] = c8[i];
  if (MODE == VGX_MARKER_COLOR || MODE == VGX_MARKER_LAMBERT_COLOR) __syncthreads();
  // one colour per triangle
  const unsigned long long t = b * kMarkerThreads + i;
  if (MODE != VGX_MARKER_HEIGHT && t < n_tris) {
    float rgb[3] = {0.5f, 0.5f, 0.5f};  // VGX_MARKER_GRAY
    float n[3];
    if (MODE == VGX_MARKER_NORMALS || MODE == VGX_MARKER_LAMBERT_COLOR) {
#pragma unroll
      for (int a = 0; a < 3; ++a) n[a] = tri_normals[3 * t + a];
    }
    float c[3];
    if (!PV && (MODE == VGX_MARKER_COLOR || MODE == VGX_MARKER_LAMBERT_COLOR)) {
      const uint32_t w = tri_colors ? tri_colors[t] : P.constant_rgba;
      c[0] = s_c8[w & 255u];
      c[1] = s_c8[(w >> 8) & 255u];
      c[2] = s_c8[(w >> 16) & 255u];
    }
    if (PV) {  // tri_colors is [3 T]: the lights here, the shading per vertex below
      if (MODE == VGX_MARKER_LAMBERT_COLOR) {
        rgb[0] = marker_light(n, P.light1);
        rgb[1] = marker_light(n, P.light2);
      }
    } else if (MODE == VGX_MARKER_COLOR) {
#pragma unroll
      for (int a = 0; a < 3; ++a) rgb[a] = c[a];
    } else if (MODE == VGX_MARKER_NORMALS) {
#pragma unroll
      for (int a = 0; a < 3; ++a) rgb[a] = (float)((double)n[a] * 0.5 + 0.5);  // (the product is exact in f64)
    } else if (MODE == VGX_MARKER_LAMBERT_COLOR) {
      const float d1 = marker_light(n, P.light1), d2 = marker_light(n, P.light2);
#pragma unroll
      for (int a = 0; a < 3; ++a) rgb[a] = marker_lambert(c[a], d1, d2);
    }
    s_colour[i] = make_float4(rgb[0], rgb[1], rgb[2], P.opacity);
  }
  __syncthreads();
  // points: float pair g of the soup -> one 16-byte store
  const unsigned long long n_floats = 9ull * n_tris;
  constexpr unsigned kPairs = 9 * kMarkerThreads / 2;  // 1152 per workgroup (2304 floats: a workgroup starts on a pair)
#pragma unroll
  for (unsigned k = 0; k < (kPairs + kMarkerThreads - 1) / kMarkerThreads; ++k) {
    const unsigned il = i + k * kMarkerThreads;
    const unsigned long long f0 = 2ull * (b * kPairs + il);
    if (il < kPairs && f0 + 1 < n_floats) {
      const float2 v = *reinterpret_cast<const float2*>(soup + f0);
      *reinterpret_cast<double2*>(points + f0) = make_double2((double)v.x, (double)v.y);
    } else if (il < kPairs && f0 < n_floats) {  // (9 T odd: the last float stands alone)
      points[f0] = (double)soup[f0];
    }
  }
  // colours: vertex j -> one 16-byte store
  const unsigned long long n_verts = 3ull * n_tris;
#pragma unroll
  for (unsigned k = 0; k < 3; ++k) {
    const unsigned jl = i + k * kMarkerThreads;
    const unsigned long long j = b * (3ull * kMarkerThreads) + jl;
    if (j >= n_verts) continue;
    if (MODE == VGX_MARKER_HEIGHT) {
      float rgb[3];
      marker_height(soup[3 * j + 2], s_c8, rgb);
      colors[j] = make_float4(rgb[0], rgb[1], rgb[2], P.opacity);
    } else if (PV) {
      const uint32_t w = tri_colors[j];
      float rgb[3] = {s_c8[w & 255u], s_c8[(w >> 8) & 255u], s_c8[(w >> 16) & 255u]};
      if (MODE == VGX_MARKER_LAMBERT_COLOR) {
        const float4 l = s_colour[jl / 3u];
#pragma unroll
        for (int a = 0; a < 3; ++a) rgb[a] = marker_lambert(rgb[a], l.x, l.y);
      }
      colors[j] = make_float4(rgb[0], rgb[1], rgb[2], P.opacity);
    } else {
      colors[j] = s_colour[jl / 3u];
    }
  }
}

}  // namespace vgx

using namespace vgx;

struct vgx_mesh_marker_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  int64_t n_points = 0;  // the marker held now
  int32_t color_mode = VGX_MARKER_LAMBERT_COLOR;
  // output, grown on demand (one capacity in vertices)
  DeviceBuffer d_points;  // double [cap][3]
  DeviceBuffer d_colors;  // float [cap][4]
  DeviceBuffer d_c8;      // float [256]: uploaded by the first fill
};

namespace {

// a quarter of slack (the next map is a little larger), at least 4096 vertices
size_t marker_capacity(int64_t n) { return (size_t)std::max<int64_t>(n + n / 4, 4096); }

// L / sqrtf((x*x + y*y) + z*z), component by component
void marker_normalised(const float L[3], float out[3]) {
  const float len = sqrtf((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]);
  for (int a = 0; a < 3; ++a) out[a] = L[a] / len;
}

const float* marker_c8_table() {
  static float table[256];
  static std::once_flag once;
  std::call_once(once, [] {
    for (int k = 0; k < 256; ++k) table[k] = (float)((double)k / 255.0);
  });
  return table;
}

// the pass over T > 0 triangles on `st` (the caller holds both handles' locks and the registration lock, and has reset
// K's stats)
int fill_marker(vgx_ctx ctx, hipStream_t st, const MeshView& src, const vgx_mesh_marker_config& cfg, vgx_mesh_marker K) {
  const int64_t n = 3 * src.n_tris;
  if ((size_t)n * 16 > K->d_colors.bytes) {
    const size_t cap = marker_capacity(n);
    const hipError_t e = alloc_group({{&K->d_points, cap * 24}, {&K->d_colors, cap * 16}});
    if (e != hipSuccess) return alloc_error(ctx, e, "mesh marker: allocating points and colours");
  }
  if (!K->d_c8.p) {
    const hipError_t e = K->d_c8.alloc(256 * sizeof(float));
    if (e != hipSuccess) return alloc_error(ctx, e, "mesh marker: allocating the channel table");
    const hipError_t c = hipMemcpyAsync(K->d_c8.p, marker_c8_table(), 256 * sizeof(float), hipMemcpyHostToDevice, st);
    if (c != hipSuccess) {
      K->d_c8.release();
      VGX_HIP(ctx, c);
    }
  }
  MarkerParams P{};
  const float L1[3] = {0.8f, -0.2f, 0.7f}, L2[3] = {-0.5f, 0.2f, 0.2f};
  marker_normalised(L1, P.light1);
  marker_normalised(L2, P.light2);
  P.opacity = cfg.opacity;
  std::memcpy(&P.constant_rgba, cfg.constant_rgba, 4);
  int mode = cfg.color_mode;
  const uint32_t* tri_colors = cfg.use_constant_color ? nullptr : src.colors;
  if (mode == VGX_MARKER_LAMBERT) {  // LAMBERT_COLOR with the colour (127, 127, 127)
    mode = VGX_MARKER_LAMBERT_COLOR;
    tri_colors = nullptr;
    const uint8_t grey[4] = {127, 127, 127, 255};
    std::memcpy(&P.constant_rgba, grey, 4);
  }
  const dim3 grid((unsigned)((src.n_tris + kMarkerThreads - 1) / kMarkerThreads)), block(kMarkerThreads);
  const unsigned long long T = (unsigned long long)src.n_tris;
  const float* c8 = K->d_c8.as<float>();
  double* points = K->d_points.as<double>();
  float4* colors = K->d_colors.as<float4>();
#define VGX_MARKER_LAUNCH(M) \
  hipLaunchKernelGGL(marker_fill_kernel<M>, grid, block, 0, st, src.vertices, src.normals, tri_colors, T, c8, P, points, colors)
  const bool pv = tri_colors && src.per_vertex;  // one colour per soup vertex: COLOR and LAMBERT_COLOR shade each apart
  if (pv && mode == VGX_MARKER_COLOR) {
    hipLaunchKernelGGL((marker_fill_kernel<VGX_MARKER_COLOR, true>), grid, block, 0, st, src.vertices, src.normals, tri_colors, T, c8, P,
                       points, colors);
  } else if (pv && mode == VGX_MARKER_LAMBERT_COLOR) {
    hipLaunchKernelGGL((marker_fill_kernel<VGX_MARKER_LAMBERT_COLOR, true>), grid, block, 0, st, src.vertices, src.normals, tri_colors, T,
                       c8, P, points, colors);
  } else {
    switch (mode) {
      case VGX_MARKER_COLOR: VGX_MARKER_LAUNCH(VGX_MARKER_COLOR); break;
      case VGX_MARKER_HEIGHT: VGX_MARKER_LAUNCH(VGX_MARKER_HEIGHT); break;
      case VGX_MARKER_NORMALS: VGX_MARKER_LAUNCH(VGX_MARKER_NORMALS); break;
      case VGX_MARKER_GRAY: VGX_MARKER_LAUNCH(VGX_MARKER_GRAY); break;
      default: VGX_MARKER_LAUNCH(VGX_MARKER_LAMBERT_COLOR); break;
    }
  }
#undef VGX_MARKER_LAUNCH
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, hipStreamSynchronize(st));
  K->n_points = n;
  return VGX_OK;
}

}  // namespace

extern "C" {

void vgx_mesh_marker_config_default(vgx_mesh_marker_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->color_mode = VGX_MARKER_LAMBERT_COLOR;
  cfg->opacity = 1.0f;
}

int vgx_mesh_marker_create(vgx_ctx ctx, vgx_mesh_marker* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_mesh_marker_create: NULL argument");
  vgx_mesh_marker K = new vgx_mesh_marker_s;
  K->ctx = ctx;
  *out = K;
  return VGX_OK;
}

int vgx_mesh_marker_destroy(vgx_mesh_marker K) {
  if (!K) return VGX_ERR_INVALID;
  (void)hipSetDevice(K->ctx->device);
  delete K;
  return VGX_OK;
}

int vgx_mesh_fill_marker(vgx_mesh M, const vgx_mesh_marker_config* cfg_in, vgx_mesh_marker K) {
  static const char* kFn = "vgx_mesh_fill_marker: ";
  if (!M) return set_error(K ? K->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + "NULL mesh");
  vgx_ctx ctx = mesh_view(M).ctx;
  if (!K) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "NULL marker");
  if (K->ctx != ctx) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "marker of another context");
  vgx_mesh_marker_config cfg;
  vgx_mesh_marker_config_default(&cfg);
  if (cfg_in) cfg = *cfg_in;
  if (cfg.color_mode < VGX_MARKER_COLOR || cfg.color_mode > VGX_MARKER_LAMBERT_COLOR)
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "unknown color_mode");
  if (!std::isfinite(cfg.opacity)) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "opacity not finite");
  std::lock_guard<std::mutex> out_lk(K->mu);
  std::lock_guard<std::mutex> mesh_lk(mesh_mutex(M));
  const MeshView src = mesh_view(M);
  if (!src.holds_mesh) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "the source handle holds no mesh (its last call failed)");
  if ((cfg.color_mode == VGX_MARKER_COLOR || cfg.color_mode == VGX_MARKER_LAMBERT_COLOR) && !cfg.use_constant_color &&
      !(src.has_colors && (src.colors || src.n_tris == 0)))
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + "the mesh has no colours (this mode needs them, or use_constant_color)");
  if (3 * src.n_tris >= ((int64_t)1 << 32))
    return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + "3 T >= 2^32 (a ROS array length is a u32)");
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  K->n_points = 0;
  K->color_mode = cfg.color_mode;
  if (src.n_tris == 0) return VGX_OK;
  return fill_marker(ctx, ctx->stream, src, cfg, K);  // (after a failure the handle holds no marker: stats report 0)
}

int vgx_mesh_marker_stats(vgx_mesh_marker K, int64_t* n_points, int32_t* color_mode) {
  if (!K) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(K->mu);
  if (n_points) *n_points = K->n_points;
  if (color_mode) *color_mode = K->color_mode;
  return VGX_OK;
}

int vgx_mesh_marker_download(vgx_mesh_marker K, double* points, float* colors) {
  if (!K) return VGX_ERR_INVALID;
  vgx_ctx ctx = K->ctx;
  std::lock_guard<std::mutex> lk(K->mu);
  if (K->n_points == 0) return VGX_OK;
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  if (points) VGX_HIP(ctx, hipMemcpy(points, K->d_points.p, (size_t)K->n_points * 24, hipMemcpyDeviceToHost));
  if (colors) VGX_HIP(ctx, hipMemcpy(colors, K->d_colors.p, (size_t)K->n_points * 16, hipMemcpyDeviceToHost));
  return VGX_OK;
}

int vgx_mesh_marker_device_pointers(vgx_mesh_marker K, const double** points, const float** colors) {
  if (!K) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(K->mu);
  const bool any = K->n_points > 0;
  if (points) *points = any ? K->d_points.as<double>() : nullptr;
  if (colors) *colors = any ? K->d_colors.as<float>() : nullptr;
  return VGX_OK;
}

}  // extern "C"
