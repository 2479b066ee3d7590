// View rendering (include/voxgraph_amd.h, "View rendering"): range images ray-marched out of a TSDF layer,
// the inverse of vgx_tsdf_integrate.  The formulation is stated in the header; tests/view_render_ref.py restates every bit.
//
//   view_kernel<VPS, LAYER>: one ray per lane, 256 threads per workgroup.  A ray is a chain of dependent samples: per
//   sample one multiply-add per axis, one block-table lookup per neighbour and 8 gathers of {distance, weight} issued
//   together; the step is a fraction of the distance read (sphere tracing), the hit a linear interpolation between the
//   last positive sample and the first that is not.  One more sample at the hit gives gradient, weight and colour.
//   The per-call counts are integer atomics, one add per count and workgroup.  No float atomics, no transcendental.
// LAYER is what a sample reads: the live layer's packed {distance, weight} words (ViewLiveLayer) or a finished submap's raw
// TSDF arrays (ViewRawLayer).  One launch, one 64-byte D2H copy into the handle's pinned stage and one synchronisation.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>

#include "vgx_internal.h"
#include "vgx_interp.h"
#include "vgx_query_kernel.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

constexpr int kViewThreads = 256;
constexpr int kViewCounts = 8;  // vgx_view_counts as int64 words
// s_max / min(min_step, unknown_step) <= 65536 (refused otherwise) bounds a ray at 65537 samples and a few more for the
// roundings of s; the loop's own bound is far above that and never binds -- it is there so that no input can hang a device
constexpr int kViewMaxSamples = 1 << 17;

// the block table, the colours (or null) and one voxel's {distance, weight}
struct ViewLiveLayer : LayerTable {
  const uint32_t* rgba;
  const unsigned long long* voxels;  // [blocks][vps^3] {distance (lo), weight (hi)}
  __device__ __forceinline__ void voxel(size_t at, float& d, float& w) const {
    const unsigned long long v = voxels[at];
    d = __uint_as_float((unsigned int)(v & 0xffffffffull));
    w = __uint_as_float((unsigned int)(v >> 32));
  }
};
struct ViewRawLayer : LayerTable {
  const uint32_t* rgba;
  const float* tsdf_d;  // [blocks][vps^3]
  const float* tsdf_w;
  __device__ __forceinline__ void voxel(size_t at, float& d, float& w) const {
    d = tsdf_d[at];
    w = tsdf_w[at];
  }
};

template <class LAYER>
struct ViewDev {
  LAYER layer;
  float q[4], t[3];  // T_L_C
  float s_min, s_max, step_scale, min_step, unknown_step, max_bracket;
  const float* dirs;  // [n][3] sensor frame
  long long n;
  long long image_width, tiles_x;  // image_width > 0: a wave takes an 8 x 8 tile of the image
  float* range;                    // [n]
  uint8_t* status;                 // [n]
  float* points;                   // [n][3] or null, as the four below
  float* gradient;
  float* weight;
  uint32_t* rgba;
  int32_t* n_samples;
  unsigned long long* counts;  // [kViewCounts], zero before the launch
};

// One sample: false when it is invalid; otherwise the 8 neighbours' distances and weights (k: x = bit 2, y = bit 1,
// z = bit 0) and the position within their cube.  The addresses first, then the gathers together.
template <int VPS, class LAYER>
__device__ __forceinline__ bool view_sample(const LAYER& L, const float (&pos)[3], float (&x)[8], float (&w)[8], float (&dl)[3]) {
  constexpr int VOX = VPS * VPS * VPS;
  // the query kernel's rule: a block coordinate outside (-2^30, 2^30) -- every non-finite position -- is invalid
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && fabsf(pos[a] * L.block_size_inv) < 1073741824.0f;
  if (!ok) return false;
  int blk[3], vox[3];
  interp_base<VPS>(L, pos, blk, vox, dl);
  // interp_neighbours' walk in this kernel's own lines: through the helper the sample loop reloaded 9 descriptor words per
  // sample, and a LiDAR view (64 x 1024 rays, one ray per lane) took 5 % longer on the MI355X
  size_t at[8];
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
    const int slot = interp_slot(L, nb[0], nb[1], nb[2]);
    ok = ok && slot >= 0;
    at[k] = (size_t)(slot >= 0 ? slot : 0) * VOX + (size_t)(nv[0] + VPS * (nv[1] + VPS * nv[2]));
  }
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    L.voxel(at[k], x[k], w[k]);
    ok = ok && interp_valid(w[k]);
  }
  return ok;
}

template <int VPS, class LAYER>
__global__ __launch_bounds__(kViewThreads) void view_kernel(ViewDev<LAYER> v) {
  __shared__ unsigned long long sh[kViewThreads / 64][kViewCounts];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long i;
  if (v.image_width > 0) {
    // wave g takes tile (g % tiles_x, g / tiles_x), lane l its pixel (l % 8, l / 8); a pixel right of the image or a
    // ray below its last row is nobody's
    const long long g = (long long)blockIdx.x * (kViewThreads / 64) + wave;
    const long long ty = g / v.tiles_x, tx = g - ty * v.tiles_x;
    const long long col = tx * 8 + (lane & 7), row = ty * 8 + (lane >> 3);
    i = col < v.image_width ? row * v.image_width + col : v.n;
  } else {
    i = (long long)blockIdx.x * kViewThreads + threadIdx.x;
  }
  const bool live = i < v.n;
  int status = VGX_VIEW_MISS, samples = 0;
  float s_hit = 0.0f, pt[3] = {0.0f, 0.0f, 0.0f}, grad[3] = {0.0f, 0.0f, 0.0f}, wgt = 0.0f;
  uint32_t colour = 0u;
  if (live) {
    const float dir[3] = {v.dirs[3 * i], v.dirs[3 * i + 1], v.dirs[3 * i + 2]};
    const bool finite = fabsf(dir[0]) < INFINITY && fabsf(dir[1]) < INFINITY && fabsf(dir[2]) < INFINITY;  // (a NaN fails)
    if (!finite || (dir[0] == 0.0f && dir[1] == 0.0f && dir[2] == 0.0f)) {
      status = VGX_VIEW_BAD;
    } else {
      float d[3];
      quat_rotate(v.q, dir, d);
      float x[8], w[8], dl[3], pos[3];
      float s = v.s_min, s0 = 0.0f, D0 = 0.0f;
      bool have = false, hit = false;
#pragma unroll 1
      for (int it = 0; it < kViewMaxSamples; ++it) {
        if (!(s <= v.s_max)) break;  // MISS
#pragma unroll
        for (int a = 0; a < 3; ++a) pos[a] = d[a] * s + v.t[a];
        ++samples;
        if (view_sample<VPS>(v.layer, pos, x, w, dl)) {
          const float D = interp_trilinear(x, dl);
          if (D > 0.0f) {
            have = true;
            s0 = s;
            D0 = D;
            const float step = D * v.step_scale;
            s = s + (step > v.min_step ? step : v.min_step);
          } else {
            if (have && (s - s0) <= v.max_bracket) {
              hit = true;
              s_hit = s0 + (s - s0) * (D0 / (D0 - D));
            } else {
              status = VGX_VIEW_INSIDE;
            }
            break;
          }
        } else {
          s = s + v.unknown_step;
        }
      }
      if (hit) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          pos[a] = d[a] * s_hit + v.t[a];
          pt[a] = dir[a] * s_hit;
        }
        ++samples;
        if (view_sample<VPS>(v.layer, pos, x, w, dl)) {
          status = VGX_VIEW_HIT;
          float gl[3];
          interp_trilinear_gradient(x, dl, gl);
#pragma unroll
          for (int a = 0; a < 3; ++a) grad[a] = gl[a] * v.layer.voxel_size_inv;
          wgt = interp_trilinear(w, dl);
          if (v.rgba && v.layer.rgba) colour = tsdf_color_interp<VPS>(v.layer, v.layer.rgba, pos);
        } else {
          status = VGX_VIEW_HIT_UNSAMPLED;
        }
      }
    }
    v.range[i] = s_hit;
    v.status[i] = (uint8_t)status;
    if (v.points) {
      v.points[3 * i] = pt[0];
      v.points[3 * i + 1] = pt[1];
      v.points[3 * i + 2] = pt[2];
    }
    if (v.gradient) {
      v.gradient[3 * i] = grad[0];
      v.gradient[3 * i + 1] = grad[1];
      v.gradient[3 * i + 2] = grad[2];
    }
    if (v.weight) v.weight[i] = wgt;
    if (v.rgba) v.rgba[i] = colour;
    if (v.n_samples) v.n_samples[i] = samples;
  }
  // the counts: ballots per status, the samples summed over the wave; lane 0 of every wave -> shared, one add per count
  unsigned long long c[kViewCounts];
  c[0] = (unsigned long long)__popcll(__ballot(live));
  c[1] = (unsigned long long)__popcll(__ballot(live && status == VGX_VIEW_HIT));
  c[2] = (unsigned long long)__popcll(__ballot(live && status == VGX_VIEW_HIT_UNSAMPLED));
  c[3] = (unsigned long long)__popcll(__ballot(live && status == VGX_VIEW_MISS));
  c[4] = (unsigned long long)__popcll(__ballot(live && status == VGX_VIEW_INSIDE));
  c[5] = (unsigned long long)__popcll(__ballot(live && status == VGX_VIEW_BAD));
  int total = samples;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_down(total, o);
  c[6] = (unsigned long long)total;
  c[7] = 0ull;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kViewCounts; ++k) sh[wave][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x < kViewCounts - 1) {
    unsigned long long sum = 0ull;
#pragma unroll
    for (int k = 0; k < kViewThreads / 64; ++k) sum += sh[k][threadIdx.x];
    if (sum) atomicAdd(v.counts + threadIdx.x, sum);
  }
}

}  // namespace vgx

using namespace vgx;

struct vgx_view_s {
  vgx_ctx ctx = nullptr;
  vgx_view_config cfg{};
  std::mutex mu;     // one call at a time per handle
  int64_t n = 0;     // rays of the view held now
  int64_t cap = 0;   // rays the output arrays hold
  // the outputs, grown together on demand; those the flags do not ask for stay empty
  DeviceBuffer d_range, d_status, d_points, d_gradient, d_weight, d_rgba, d_n_samples;
  DeviceBuffer d_dirs;    // the host-pointer calls' copy of the directions
  DeviceBuffer d_counts;  // vgx_view_counts
  PinnedBuffer h_counts;  // ... and their pinned stage
  vgx_view_counts counts{};
};

namespace {

int view_fail(vgx_ctx ctx, const char* fn, const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": " + msg); }

const char* view_config_error(const vgx_view_config& c) {
  for (float f : {c.s_min, c.s_max, c.step_scale, c.min_step, c.unknown_step, c.max_bracket})
    if (!std::isfinite(f)) return "a field is not finite";
  if (c.s_min < 0.0f) return "s_min < 0";
  if (!(c.s_max > 0.0f)) return "s_max must be positive (it has no default)";
  if (c.s_min > c.s_max) return "s_min > s_max";
  if (!(c.step_scale > 0.0f)) return "step_scale <= 0";
  if (!(c.min_step > 0.0f) || !(c.unknown_step > 0.0f)) return "min_step and unknown_step must be positive (they have no default)";
  if (!(c.max_bracket > 0.0f)) return "max_bracket must be positive (it has no default)";
  if ((double)c.s_max / (double)std::min(c.min_step, c.unknown_step) > 65536.0) return "s_max / min(min_step, unknown_step) > 65536";
  if (c.image_width < 0) return "image_width < 0";
  if (c.flags & ~VGX_VIEW_ALL) return "unknown flag bits";
  return nullptr;
}

// what every render call refuses before any lock; `layer_ctx` null: a NULL layer or submap
int view_check(const char* fn, vgx_view V, vgx_ctx layer_ctx, const float* T, int64_t n, const void* dirs) {
  vgx_ctx ctx = V->ctx;
  if (!layer_ctx || !T) return view_fail(ctx, fn, "NULL layer or pose");
  if (layer_ctx != ctx) return view_fail(ctx, fn, "the layer belongs to another context");
  if (n < 0 || (n > 0 && !dirs)) return view_fail(ctx, fn, "n < 0 or NULL directions");
  const PoseDefect bad = pose_defect(T);
  if (bad == kPoseNotFinite) return view_fail(ctx, fn, "the pose is not finite");
  if (bad == kPoseNotUnit) return view_fail(ctx, fn, "the pose's quaternion is not unit (| |q|^2 - 1 | > 1e-4)");
  return VGX_OK;
}

// workgroups of a launch over n rays; the tiles of a row in *tiles_x
int64_t view_groups(int64_t n, int64_t image_width, int64_t* tiles_x) {
  *tiles_x = 0;
  if (image_width <= 0) return (n + kViewThreads - 1) / kViewThreads;
  const int64_t rows = (n + image_width - 1) / image_width;
  *tiles_x = (image_width + 7) / 8;
  const int64_t tiles = *tiles_x * ((rows + 7) / 8);
  return (tiles + kViewThreads / 64 - 1) / (kViewThreads / 64);
}

int view_reserve(vgx_view V, int64_t n) {
  if (n > V->cap) {
    const int32_t f = V->cfg.flags;
    const size_t un = (size_t)n;
    V->cap = 0;
    const hipError_t e = alloc_group({{&V->d_range, un * 4},
                                      {&V->d_status, un},
                                      {&V->d_points, (f & VGX_VIEW_POINTS) ? un * 12 : 0},
                                      {&V->d_gradient, (f & VGX_VIEW_GRADIENT) ? un * 12 : 0},
                                      {&V->d_weight, (f & VGX_VIEW_WEIGHT) ? un * 4 : 0},
                                      {&V->d_rgba, (f & VGX_VIEW_RGBA) ? un * 4 : 0},
                                      {&V->d_n_samples, (f & VGX_VIEW_N_SAMPLES) ? un * 4 : 0}});
    if (e != hipSuccess) return alloc_error(V->ctx, e, "vgx_view: allocating the outputs");
    V->cap = n;
  }
  if (!V->d_counts.p) {
    const hipError_t e = V->d_counts.alloc(sizeof(vgx_view_counts));
    if (e != hipSuccess) return alloc_error(V->ctx, e, "vgx_view: allocating the counts");
  }
  if (!V->h_counts.p) {
    const hipError_t e = V->h_counts.alloc(sizeof(vgx_view_counts));
    if (e != hipSuccess) return alloc_error(V->ctx, e, "vgx_view: allocating the pinned stage");
  }
  return VGX_OK;
}

// One view on stream st: V->mu and the stream's lock held, the device set, n > 0.  `layer` holds everything but the
// pose, the directions and the outputs.
template <class LAYER>
int view_render_locked(vgx_view V, hipStream_t st, int vps, const LAYER& layer, const float T[7], int64_t n, const void* dirs,
                       bool host) {
  vgx_ctx ctx = V->ctx;
  V->n = 0;  // (what a failure below leaves)
  std::memset(&V->counts, 0, sizeof(V->counts));
  int rc = view_reserve(V, n);
  if (rc != VGX_OK) return rc;
  if (host) {
    const hipError_t e = V->d_dirs.reserve((size_t)n * 12, 0, true);
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_view: allocating the directions");
    VGX_HIP(ctx, hipMemcpyAsync(V->d_dirs.p, dirs, (size_t)n * 12, hipMemcpyHostToDevice, st));
  }
  ViewDev<LAYER> d{};
  d.layer = layer;
  for (int k = 0; k < 4; ++k) d.q[k] = T[k];
  for (int a = 0; a < 3; ++a) d.t[a] = T[4 + a];
  const vgx_view_config& c = V->cfg;
  d.s_min = c.s_min;
  d.s_max = c.s_max;
  d.step_scale = c.step_scale;
  d.min_step = c.min_step;
  d.unknown_step = c.unknown_step;
  d.max_bracket = c.max_bracket;
  d.dirs = host ? V->d_dirs.as<float>() : static_cast<const float*>(dirs);
  d.n = n;
  d.image_width = c.image_width;
  int64_t tiles_x = 0;
  const int64_t groups = view_groups(n, c.image_width, &tiles_x);
  d.tiles_x = tiles_x;
  d.range = V->d_range.as<float>();
  d.status = V->d_status.as<uint8_t>();
  d.points = (c.flags & VGX_VIEW_POINTS) ? V->d_points.as<float>() : nullptr;
  d.gradient = (c.flags & VGX_VIEW_GRADIENT) ? V->d_gradient.as<float>() : nullptr;
  d.weight = (c.flags & VGX_VIEW_WEIGHT) ? V->d_weight.as<float>() : nullptr;
  d.rgba = (c.flags & VGX_VIEW_RGBA) ? V->d_rgba.as<uint32_t>() : nullptr;
  d.n_samples = (c.flags & VGX_VIEW_N_SAMPLES) ? V->d_n_samples.as<int32_t>() : nullptr;
  d.counts = V->d_counts.as<unsigned long long>();
  VGX_HIP(ctx, hipMemsetAsync(V->d_counts.p, 0, sizeof(vgx_view_counts), st));
  if (vps == 16)
    hipLaunchKernelGGL((view_kernel<16, LAYER>), dim3((unsigned)groups), dim3(kViewThreads), 0, st, d);
  else
    hipLaunchKernelGGL((view_kernel<8, LAYER>), dim3((unsigned)groups), dim3(kViewThreads), 0, st, d);
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, hipMemcpyAsync(V->h_counts.p, V->d_counts.p, sizeof(vgx_view_counts), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  V->counts = *V->h_counts.as<vgx_view_counts>();
  V->n = n;
  return VGX_OK;
}

int view_too_large(vgx_view V, const char* fn, int64_t n) {
  int64_t tiles_x = 0;
  if (view_groups(n, V->cfg.image_width, &tiles_x) > 0x7fffffffll)
    return set_error(V->ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": too many rays for one launch");
  return VGX_OK;
}

// n = 0: the view holds no ray
int view_empty(vgx_view V) {
  std::lock_guard<std::mutex> lk(V->mu);
  V->n = 0;
  std::memset(&V->counts, 0, sizeof(V->counts));
  return VGX_OK;
}

int layer_render(const char* fn, vgx_tsdf_layer L, vgx_view V, const float* T, int64_t n, const void* dirs, bool host) {
  if (!V) return VGX_ERR_INVALID;
  vgx_ctx ctx = V->ctx;
  int rc = view_check(fn, V, L ? L->ctx : nullptr, T, n, dirs);
  if (rc != VGX_OK) return rc;
  if (L->dev.vps != 8 && L->dev.vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": voxels_per_side not 8 or 16");
  rc = view_too_large(V, fn, n);
  if (rc != VGX_OK) return rc;
  if (n == 0) return view_empty(V);
  std::lock_guard<std::mutex> lk(V->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const TsdfLayerDev& ld = L->dev;
  ViewLiveLayer layer{};
  static_cast<LayerTable&>(layer) = live_layer_table(L);
  layer.rgba = ld.rgba;
  layer.voxels = ld.voxels;
  return view_render_locked(V, ctx->tsdf_stream, ld.vps, layer, T, n, dirs, host);
}

int submap_render(const char* fn, vgx_submap sm, vgx_view V, const float* T, int64_t n, const void* dirs, bool host) {
  if (!V) return VGX_ERR_INVALID;
  vgx_ctx ctx = V->ctx;
  int rc = view_check(fn, V, sm ? sm->ctx : nullptr, T, n, dirs);
  if (rc != VGX_OK) return rc;
  if (sm->n_blocks > 0 && !(sm->d_tsdf_distance && sm->d_tsdf_weight))
    return view_fail(ctx, fn, "TSDF layer not resident (released by vgx_submap_release_raw_layers)");
  if (sm->vps != 8 && sm->vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": voxels_per_side not 8 or 16");
  rc = view_too_large(V, fn, n);
  if (rc != VGX_OK) return rc;
  if (n == 0) return view_empty(V);
  std::lock_guard<std::mutex> lk(V->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  ViewRawLayer layer{};
  static_cast<LayerTable&>(layer) = submap_table(sm);
  layer.rgba = sm->d_tsdf_rgba;
  layer.tsdf_d = sm->d_tsdf_distance;
  layer.tsdf_w = sm->d_tsdf_weight;
  return view_render_locked(V, ctx->stream, sm->vps, layer, T, n, dirs, host);
}

int rays_check(int32_t width, int32_t height, const float* dirs) { return width >= 1 && height >= 1 && dirs ? VGX_OK : VGX_ERR_INVALID; }

}  // namespace

extern "C" {

void vgx_view_config_default(vgx_view_config* cfg) {
  if (!cfg) return;
  cfg->s_min = 0.0f;
  cfg->s_max = 0.0f;  // (no default: the caller states it, and the three below)
  cfg->step_scale = 0.75f;
  cfg->min_step = 0.0f;
  cfg->unknown_step = 0.0f;
  cfg->max_bracket = 0.0f;
  cfg->image_width = 0;
  cfg->flags = VGX_VIEW_POINTS;
}

int vgx_view_config_check(const vgx_view_config* cfg) { return cfg && !view_config_error(*cfg) ? VGX_OK : VGX_ERR_INVALID; }

int vgx_view_create(vgx_ctx ctx, const vgx_view_config* cfg, vgx_view* out) {
  const char* fn = "vgx_view_create";
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL context or output");
  *out = nullptr;
  if (!cfg) return view_fail(ctx, fn, "NULL config (s_max, min_step, unknown_step and max_bracket have no default)");
  if (const char* why = view_config_error(*cfg)) return view_fail(ctx, fn, why);
  vgx_view V = new (std::nothrow) vgx_view_s;
  if (!V) return set_error(ctx, VGX_ERR_NOMEM, std::string(fn) + ": out of host memory");
  V->ctx = ctx;
  V->cfg = *cfg;
  *out = V;
  return VGX_OK;
}

int vgx_view_destroy(vgx_view V) {
  if (!V) return VGX_ERR_INVALID;
  (void)hipSetDevice(V->ctx->device);  // (every render ended with a synchronisation: nothing queued reads the arrays)
  delete V;
  return VGX_OK;
}

int vgx_view_stats(vgx_view V, vgx_view_counts* counts) {
  if (!V) return VGX_ERR_INVALID;
  if (!counts) return view_fail(V->ctx, "vgx_view_stats", "NULL counts");
  std::lock_guard<std::mutex> lk(V->mu);
  *counts = V->counts;
  return VGX_OK;
}

int vgx_view_device_pointers(vgx_view V, const float** range, const uint8_t** status, const float** points, const float** gradient,
                             const float** weight, const uint32_t** rgba, const int32_t** n_samples) {
  if (!V) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(V->mu);
  const bool any = V->n > 0;
  const int32_t f = V->cfg.flags;
  if (range) *range = any ? V->d_range.as<float>() : nullptr;
  if (status) *status = any ? V->d_status.as<uint8_t>() : nullptr;
  if (points) *points = any && (f & VGX_VIEW_POINTS) ? V->d_points.as<float>() : nullptr;
  if (gradient) *gradient = any && (f & VGX_VIEW_GRADIENT) ? V->d_gradient.as<float>() : nullptr;
  if (weight) *weight = any && (f & VGX_VIEW_WEIGHT) ? V->d_weight.as<float>() : nullptr;
  if (rgba) *rgba = any && (f & VGX_VIEW_RGBA) ? V->d_rgba.as<uint32_t>() : nullptr;
  if (n_samples) *n_samples = any && (f & VGX_VIEW_N_SAMPLES) ? V->d_n_samples.as<int32_t>() : nullptr;
  return VGX_OK;
}

int vgx_view_download(vgx_view V, float* range, uint8_t* status, float* points, float* gradient, float* weight, uint32_t* rgba,
                      int32_t* n_samples) {
  if (!V) return VGX_ERR_INVALID;
  vgx_ctx ctx = V->ctx;
  std::lock_guard<std::mutex> lk(V->mu);
  const int32_t f = V->cfg.flags;
  if ((points && !(f & VGX_VIEW_POINTS)) || (gradient && !(f & VGX_VIEW_GRADIENT)) || (weight && !(f & VGX_VIEW_WEIGHT)) ||
      (rgba && !(f & VGX_VIEW_RGBA)) || (n_samples && !(f & VGX_VIEW_N_SAMPLES)))
    return view_fail(ctx, "vgx_view_download", "an output the view's flags do not hold");
  if (V->n == 0) return VGX_OK;
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the view was complete when its render returned, whichever stream made it)
  const size_t n = (size_t)V->n;
  if (range) VGX_HIP(ctx, hipMemcpyAsync(range, V->d_range.p, n * 4, hipMemcpyDeviceToHost, st));
  if (status) VGX_HIP(ctx, hipMemcpyAsync(status, V->d_status.p, n, hipMemcpyDeviceToHost, st));
  if (points) VGX_HIP(ctx, hipMemcpyAsync(points, V->d_points.p, n * 12, hipMemcpyDeviceToHost, st));
  if (gradient) VGX_HIP(ctx, hipMemcpyAsync(gradient, V->d_gradient.p, n * 12, hipMemcpyDeviceToHost, st));
  if (weight) VGX_HIP(ctx, hipMemcpyAsync(weight, V->d_weight.p, n * 4, hipMemcpyDeviceToHost, st));
  if (rgba) VGX_HIP(ctx, hipMemcpyAsync(rgba, V->d_rgba.p, n * 4, hipMemcpyDeviceToHost, st));
  if (n_samples) VGX_HIP(ctx, hipMemcpyAsync(n_samples, V->d_n_samples.p, n * 4, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  return VGX_OK;
}

int vgx_tsdf_layer_render_view(vgx_tsdf_layer L, vgx_view V, const float T_L_C[7], int64_t n, const float* dirs) {
  return layer_render("vgx_tsdf_layer_render_view", L, V, T_L_C, n, dirs, true);
}

int vgx_tsdf_layer_render_view_device(vgx_tsdf_layer L, vgx_view V, const float T_L_C[7], int64_t n, const void* d_dirs) {
  return layer_render("vgx_tsdf_layer_render_view_device", L, V, T_L_C, n, d_dirs, false);
}

int vgx_submap_render_view(vgx_submap sm, vgx_view V, const float T_S_C[7], int64_t n, const float* dirs) {
  return submap_render("vgx_submap_render_view", sm, V, T_S_C, n, dirs, true);
}

int vgx_submap_render_view_device(vgx_submap sm, vgx_view V, const float T_S_C[7], int64_t n, const void* d_dirs) {
  return submap_render("vgx_submap_render_view_device", sm, V, T_S_C, n, d_dirs, false);
}

int vgx_view_rays_pinhole(int32_t width, int32_t height, double fx, double fy, double cx, double cy, float* dirs) {
  if (rays_check(width, height, dirs) != VGX_OK) return VGX_ERR_INVALID;
  if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy) || fx == 0.0 || fy == 0.0) return VGX_ERR_INVALID;
  for (int32_t r = 0; r < height; ++r)
    for (int32_t c = 0; c < width; ++c) {
      const double x = ((double)c - cx) / fx, y = ((double)r - cy) / fy;
      const double norm = std::sqrt((x * x + y * y) + 1.0);
      float* o = dirs + 3 * ((size_t)r * width + c);
      o[0] = (float)(x / norm);
      o[1] = (float)(y / norm);
      o[2] = (float)(1.0 / norm);
    }
  return VGX_OK;
}

int vgx_view_rays_lidar(int32_t width, int32_t height, double elevation_min, double elevation_max, double azimuth_offset, float* dirs) {
  if (rays_check(width, height, dirs) != VGX_OK) return VGX_ERR_INVALID;
  if (!std::isfinite(elevation_min) || !std::isfinite(elevation_max) || !std::isfinite(azimuth_offset)) return VGX_ERR_INVALID;
  for (int32_t r = 0; r < height; ++r) {
    const double el = height > 1 ? elevation_min + (double)r * (elevation_max - elevation_min) / (double)(height - 1) : elevation_min;
    for (int32_t c = 0; c < width; ++c) {
      const double az = (-M_PI + azimuth_offset) + (double)c * (2.0 * M_PI) / (double)width;
      float* o = dirs + 3 * ((size_t)r * width + c);
      o[0] = (float)(std::cos(el) * std::cos(az));
      o[1] = (float)(std::cos(el) * std::sin(az));
      o[2] = (float)std::sin(el);
    }
  }
  return VGX_OK;
}

}  // extern "C"
