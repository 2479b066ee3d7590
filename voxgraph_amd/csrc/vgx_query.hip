// Map queries on the device: voxblox's EsdfMap / TsdfMap lookups [recalled] -- getDistanceAtPosition,
// getDistanceAndGradientAtPosition, isObserved, getWeightAtPosition and their batch forms -- at arbitrary points of a
// finished submap's raw ESDF or TSDF layer (vgx_submap_query / _device).  The rules are stated in include/voxgraph_amd.h;
// the kernel is vgx_query_kernel.h (one thread per query, one launch per call); the layout read, the window route and
// their measurement in DESIGN.md 14.
#include "vgx_query_kernel.h"

#pragma clang fp contract(off)

using namespace vgx;

namespace {

// The window route of the interpolated gradient.  A build with -DVGX_QUERY_GENERIC_ROUTE (make SUFFIX=_generic
// EXTRA=-DVGX_QUERY_GENERIC_ROUTE: profiles/map_query_bench.py) takes the generic route alone, for timing the two against
// each other; the results are the same bits.
#ifdef VGX_QUERY_GENERIC_ROUTE
constexpr bool kWindowRoute = false;
#else
constexpr bool kWindowRoute = true;
#endif

int query_run(vgx_submap sm, int32_t layer, int32_t flags, const float* T_Q_S, int64_t n, const float* points,
              float* distance, float* gradient, float* weight, uint8_t* valid, bool host) {
  QueryDev q;
  bool run = false;
  const int rc = query_prepare(sm, layer, flags, T_Q_S, n, points, distance, gradient, weight, valid, q, run);
  if (rc != VGX_OK || !run) return rc;
  vgx_ctx ctx = sm->ctx;
  const bool tsdf = layer == VGX_EVAL_LAYER_TSDF, grad = (flags & VGX_QUERY_GRADIENT) != 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DeviceBuffer d_pts, d_dist, d_grad, d_wgt, d_valid;
  const size_t un = (size_t)n;
  if (host) {
    VGX_HIP(ctx, d_pts.alloc(un * 12));
    VGX_HIP(ctx, d_dist.alloc(un * 4));
    VGX_HIP(ctx, d_valid.alloc(un));
    if (grad) VGX_HIP(ctx, d_grad.alloc(un * 12));
    if (weight) VGX_HIP(ctx, d_wgt.alloc(un * 4));
    VGX_HIP(ctx, hipMemcpyAsync(d_pts.p, points, un * 12, hipMemcpyHostToDevice, st));
    q.points = d_pts.as<float>();
    q.distance = d_dist.as<float>();
    q.gradient = d_grad.as<float>();
    q.weight = d_wgt.as<float>();
    q.valid = d_valid.as<uint8_t>();
  } else {
    q.points = points;
    q.distance = distance;
    q.gradient = grad ? gradient : nullptr;
    q.weight = weight;
    q.valid = valid;
  }
  VGX_HIP(ctx, launch_query<kWindowRoute>(st, q, sm->vps, tsdf, (flags & VGX_QUERY_INTERPOLATE) != 0, grad));
  if (!host) return VGX_OK;
  VGX_HIP(ctx, hipMemcpyAsync(distance, d_dist.p, un * 4, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipMemcpyAsync(valid, d_valid.p, un, hipMemcpyDeviceToHost, st));
  if (grad) VGX_HIP(ctx, hipMemcpyAsync(gradient, d_grad.p, un * 12, hipMemcpyDeviceToHost, st));
  if (weight) VGX_HIP(ctx, hipMemcpyAsync(weight, d_wgt.p, un * 4, hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  return VGX_OK;
}

}  // namespace

extern "C" int vgx_submap_query(vgx_submap submap, int32_t layer, int32_t flags, const float T_Q_S[7], int64_t n,
                                const float* points, float* distance, float* gradient, float* weight, uint8_t* valid) {
  return query_run(submap, layer, flags, T_Q_S, n, points, distance, gradient, weight, valid, true);
}

extern "C" int vgx_submap_query_device(vgx_submap submap, int32_t layer, int32_t flags, const float T_Q_S[7], int64_t n,
                                       const float* points, float* distance, float* gradient, float* weight,
                                       uint8_t* valid) {
  return query_run(submap, layer, flags, T_Q_S, n, points, distance, gradient, weight, valid, false);
}
