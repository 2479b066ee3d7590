// View rendering for the mapper: what the active layer, the projected map or a finished submap looks like from a pose --
// a range image with the surface point, gradient, weight and colour per ray.  NOT a mirror of a reference class: voxblox
// has no ray caster over a layer, the formulation is the library's own (include/voxgraph_amd.h, "View rendering";
// DESIGN.md 27).  A synthetic scan rendered at a prior plugs into the registerer and the integrator as it stands:
//
//   GpuViewRenderer renderer(ctx, GpuViewRenderer::defaultConfig(16.0f, 0.05f, 0.2f, 0.6f));
//   renderer.setRays(dirs.data(), n);                         // e.g. GpuViewRenderer::lidarRays(1024, 64, -0.4, 0.3)
//   renderer.render(projected_map, T_L_C);                    // on the TSDF stream, behind every scan queued
//   renderer.renderInto(&registerer, T_prior, T_refined);     // the view's points, by device pointer, registered
//                                                             // (its min_range_m > 0 drops the rays without a hit)
#ifndef VOXGRAPH_AMD_CPP_GPU_VIEW_RENDERER_H_
#define VOXGRAPH_AMD_CPP_GPU_VIEW_RENDERER_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gpu_fast_tsdf_integrator.h"
#include "gpu_scan_to_map_registerer.h"
#include "voxgraph_amd.h"

namespace voxgraph_amd {

class GpuViewRenderer {
 public:
  using Config = vgx_view_config;
  // the defaults with the four fields that have none, all in units of |dir| (metres for unit directions): the reach, the
  // smallest step (e.g. voxel_size / 4), the step through unknown space (e.g. voxel_size) and the widest gap a hit is
  // interpolated over (e.g. the layer's truncation distance)
  static Config defaultConfig(float s_max, float min_step, float unknown_step, float max_bracket) {
    Config c;
    vgx_view_config_default(&c);
    c.s_max = s_max;
    c.min_step = min_step;
    c.unknown_step = unknown_step;
    c.max_bracket = max_bracket;
    return c;
  }
  // unit directions [height][width][3], computed in f64 and rounded once (vgx_view_rays_pinhole / _lidar)
  static std::vector<float> pinholeRays(int32_t width, int32_t height, double fx, double fy, double cx, double cy) {
    std::vector<float> dirs(3 * (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0));
    if (vgx_view_rays_pinhole(width, height, fx, fy, cx, cy, dirs.data()) != VGX_OK) throw std::invalid_argument("pinholeRays: refused");
    return dirs;
  }
  static std::vector<float> lidarRays(int32_t width, int32_t height, double elevation_min, double elevation_max,
                                      double azimuth_offset = 0.0) {
    std::vector<float> dirs(3 * (size_t)(width > 0 ? width : 0) * (size_t)(height > 0 ? height : 0));
    if (vgx_view_rays_lidar(width, height, elevation_min, elevation_max, azimuth_offset, dirs.data()) != VGX_OK)
      throw std::invalid_argument("lidarRays: refused");
    return dirs;
  }

  GpuViewRenderer(vgx_ctx ctx, const Config& config) : ctx_(ctx) {
    if (vgx_view_create(ctx, &config, &view_) != VGX_OK) throw std::runtime_error(std::string("vgx_view_create: ") + vgx_last_error(ctx));
  }
  ~GpuViewRenderer() { vgx_view_destroy(view_); }
  GpuViewRenderer(const GpuViewRenderer&) = delete;
  GpuViewRenderer& operator=(const GpuViewRenderer&) = delete;
  vgx_view handle() const { return view_; }

  // the ray directions of the renders to come: host [n][3] f32 in the sensor frame (copied; never normalised)
  void setRays(const float* dirs, int64_t n) { dirs_.assign(dirs, dirs + 3 * (size_t)(n > 0 ? n : 0)); }
  void setRays(std::vector<float> dirs) { dirs_ = std::move(dirs); }
  int64_t numRays() const { return (int64_t)(dirs_.size() / 3); }

  // the active layer or the projected map, pose {qw,qx,qy,qz, tx,ty,tz} in the layer's frame
  const vgx_view_counts& render(const GpuTsdfLayer& layer, const float T_L_C[7]) {
    if (vgx_tsdf_layer_render_view(layer.handle(), view_, T_L_C, numRays(), dirs_.data()) != VGX_OK)
      throw std::runtime_error(std::string("vgx_tsdf_layer_render_view: ") + vgx_last_error(ctx_));
    return readCounts();
  }
  // a finished submap's raw TSDF layer, pose in the submap's frame
  const vgx_view_counts& render(vgx_submap submap, const float T_S_C[7]) {
    if (vgx_submap_render_view(submap, view_, T_S_C, numRays(), dirs_.data()) != VGX_OK)
      throw std::runtime_error(std::string("vgx_submap_render_view: ") + vgx_last_error(ctx_));
    return readCounts();
  }
  // ... and with the pose as kindr::minimal::QuatTransformationTemplate<float> (getRotation().{w,x,y,z}(), getPosition()[k])
  template <class Source, class Transformation, class = decltype(std::declval<const Transformation&>().getRotation())>
  const vgx_view_counts& render(const Source& layer_or_submap, const Transformation& T_L_C) {
    const auto& q = T_L_C.getRotation();
    const auto& t = T_L_C.getPosition();
    const float T[7] = {(float)q.w(), (float)q.x(), (float)q.y(), (float)q.z(), (float)t[0], (float)t[1], (float)t[2]};
    return render(layer_or_submap, T);
  }

  const vgx_view_counts& lastCounts() const { return counts_; }

  // every array nullable; range [n], status [n], points / gradient [n][3], weight [n], rgba [n], n_samples [n]
  void download(float* range, uint8_t* status, float* points = nullptr, float* gradient = nullptr, float* weight = nullptr,
                uint32_t* rgba = nullptr, int32_t* n_samples = nullptr) const {
    if (vgx_view_download(view_, range, status, points, gradient, weight, rgba, n_samples) != VGX_OK)
      throw std::runtime_error(std::string("vgx_view_download: ") + vgx_last_error(ctx_));
  }
  // the view's sensor-frame points on the device ([n][3] f32, zeros where a ray has no hit); null without VGX_VIEW_POINTS
  const float* devicePoints() const {
    const float* p = nullptr;
    if (vgx_view_device_pointers(view_, nullptr, nullptr, &p, nullptr, nullptr, nullptr, nullptr) != VGX_OK)
      throw std::runtime_error("vgx_view_device_pointers failed");
    return p;
  }

  // The synthetic scan into scan-to-map registration (GpuScanToMapRegisterer::refineSensorPoseDevice): the registerer
  // borrows the view's points until its next scan; a later render that grows the view invalidates them.  Its config needs
  // min_range_m > 0 to leave the rays without a hit out.  Returns `usable`.
  bool renderInto(GpuScanToMapRegisterer* registerer, const float T_S_C_prior[7], float T_S_C_refined[7]) const {
    return registerer->refineSensorPoseDevice(devicePoints(), counts_.n_rays, T_S_C_prior, T_S_C_refined);
  }
  // ... and into an integrator at sensor pose T_G_C, queued behind the render (min_ray_length_m > 0 drops the rays
  // without a hit)
  void renderInto(GpuFastTsdfIntegrator* integrator, const float T_G_C[7]) const {
    if (vgx_tsdf_integrate_device(integrator->handle(), T_G_C, devicePoints(), nullptr, counts_.n_rays, 0, nullptr) != VGX_OK)
      throw std::runtime_error(std::string("vgx_tsdf_integrate_device: ") + vgx_last_error(ctx_));
  }

 private:
  const vgx_view_counts& readCounts() {
    if (vgx_view_stats(view_, &counts_) != VGX_OK) throw std::runtime_error("vgx_view_stats failed");
    return counts_;
  }

  vgx_ctx ctx_;
  vgx_view view_ = nullptr;
  std::vector<float> dirs_;
  vgx_view_counts counts_{};
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_VIEW_RENDERER_H_
