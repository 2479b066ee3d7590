// Scan-to-map registration for the mapper's frontend: the refinement voxgraph_mapper.h:164 announces ("Map tracker
// handles the odometry input and refines it using scan-to-map ICP") and the reference's MapTracker does not perform.
// NOT a mirror of a reference class: the formulation is the library's own (include/voxgraph_amd.h, "Scan-to-map
// registration").  It stands beside GpuPointcloudIntegrator, which it does not change:
//
//   // voxgraph_mapper.cpp:248-249, with the refinement in front
//   registerer.refineSensorPose(integrator.scan(), T_S_C, &T_S_C);      // keeps T_S_C when the scan cannot be registered
//   integrator.integratePointcloud7(msg, T_S_C, &layer);
//
// (INTEGRATION.md shows the order of the decode.)  Runs on the context's TSDF stream, behind every scan already queued.
#ifndef VOXGRAPH_AMD_CPP_GPU_SCAN_TO_MAP_REGISTERER_H_
#define VOXGRAPH_AMD_CPP_GPU_SCAN_TO_MAP_REGISTERER_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

#include "gpu_fast_tsdf_integrator.h"
#include "voxgraph_amd.h"

namespace voxgraph_amd {

class GpuScanToMapRegisterer {
 public:
  using Config = vgx_scan_registration_config;
  // the defaults with the one field that has none: |D| at or beyond it says nothing about the pose (below the layer's
  // truncation distance)
  static Config defaultConfig(float max_abs_distance_m) {
    Config c;
    vgx_scan_registration_config_default(&c);
    c.max_abs_distance_m = max_abs_distance_m;
    return c;
  }

  GpuScanToMapRegisterer(vgx_ctx ctx, const Config& config, GpuTsdfLayer* layer = nullptr) : ctx_(ctx), layer_(layer) {
    vgx_pose_graph_options_default(&options_);
    if (vgx_scan_registration_create(ctx, &config, &reg_) != VGX_OK)
      throw std::runtime_error(std::string("vgx_scan_registration_create: ") + vgx_last_error(ctx));
  }
  ~GpuScanToMapRegisterer() { vgx_scan_registration_destroy(reg_); }
  GpuScanToMapRegisterer(const GpuScanToMapRegisterer&) = delete;
  GpuScanToMapRegisterer& operator=(const GpuScanToMapRegisterer&) = delete;
  vgx_scan_registration handle() const { return reg_; }

  // the active submap's layer (it changes when a new submap starts, as the integrator's does)
  void setLayer(GpuTsdfLayer* layer) { layer_ = layer; }
  void setSolverOptions(const vgx_pose_graph_options& options) { options_ = options; }

  // a decoded scan (GpuPointcloudIntegrator::scan()): borrowed, it never leaves the device.  Returns `usable`;
  // *T_S_C_refined is the refined pose then, and T_S_C_prior's bits otherwise.  The two may be the same array.
  bool refineSensorPose(vgx_scan scan, const float T_S_C_prior[7], float T_S_C_refined[7]) {
    if (vgx_scan_registration_set_scan(reg_, scan) != VGX_OK)
      throw std::runtime_error(std::string("vgx_scan_registration_set_scan: ") + vgx_last_error(ctx_));
    return refine(T_S_C_prior, T_S_C_refined);
  }
  // host points [n][3] f32, sensor frame (copied)
  bool refineSensorPose(const float* points_C, int64_t n_points, const float T_S_C_prior[7], float T_S_C_refined[7]) {
    if (vgx_scan_registration_set_points(reg_, points_C, n_points) != VGX_OK)
      throw std::runtime_error(std::string("vgx_scan_registration_set_points: ") + vgx_last_error(ctx_));
    return refine(T_S_C_prior, T_S_C_refined);
  }
  // device points [n][3] f32, sensor frame, ready with respect to the TSDF stream (borrowed): a rendered view's points
  // (GpuViewRenderer::renderInto)
  bool refineSensorPoseDevice(const void* d_points_C, int64_t n_points, const float T_S_C_prior[7], float T_S_C_refined[7]) {
    if (vgx_scan_registration_set_points_device(reg_, d_points_C, n_points) != VGX_OK)
      throw std::runtime_error(std::string("vgx_scan_registration_set_points_device: ") + vgx_last_error(ctx_));
    return refine(T_S_C_prior, T_S_C_refined);
  }
  // voxblox::Pointcloud (AlignedVector<Eigen::Vector3f>: contiguous 12-byte elements), poses as {qw,qx,qy,qz, tx,ty,tz}
  template <class Pointcloud, class = typename Pointcloud::value_type>
  bool refineSensorPose(const Pointcloud& points_C, const float T_S_C_prior[7], float T_S_C_refined[7]) {
    static_assert(sizeof(typename Pointcloud::value_type) == 12, "Pointcloud: three packed floats per point");
    return refineSensorPose(reinterpret_cast<const float*>(points_C.data()), (int64_t)points_C.size(), T_S_C_prior, T_S_C_refined);
  }
  // ... and as kindr::minimal::QuatTransformationTemplate<float> (getRotation().{w,x,y,z}(), getPosition()[k], a
  // constructor from (Rotation, Position)): *T_S_C_refined is assigned only when the scan was registered
  template <class Source, class Transformation, class = decltype(std::declval<const Transformation&>().getRotation())>
  bool refineSensorPose(const Source& scan_or_pointcloud, const Transformation& T_S_C_prior, Transformation* T_S_C_refined) {
    const auto& q = T_S_C_prior.getRotation();
    const auto& t = T_S_C_prior.getPosition();
    const float T[7] = {(float)q.w(), (float)q.x(), (float)q.y(), (float)q.z(), (float)t[0], (float)t[1], (float)t[2]};
    float R[7];
    const bool usable = refineSensorPose(scan_or_pointcloud, T, R);
    if (usable && T_S_C_refined) {
      using Rotation = typename std::decay<decltype(q)>::type;
      using Position = typename std::decay<decltype(t)>::type;
      *T_S_C_refined = Transformation(Rotation(R[0], R[1], R[2], R[3]), Position(R[4], R[5], R[6]));
    } else if (T_S_C_refined) {
      *T_S_C_refined = T_S_C_prior;
    }
    return usable;
  }

  const vgx_scan_registration_summary& lastSummary() const { return summary_; }
  const double* lastCorrection() const { return delta_; }  // (x, y, z, yaw) about the sensor's prior position

 private:
  bool refine(const float T_S_C_prior[7], float T_S_C_refined[7]) {
    if (!layer_) throw std::invalid_argument("refineSensorPose: no layer set");
    if (!T_S_C_prior || !T_S_C_refined) throw std::invalid_argument("refineSensorPose: NULL pose");
    float out[7];
    if (vgx_scan_registration_refine(reg_, layer_->handle(), T_S_C_prior, &options_, out, delta_, &summary_) != VGX_OK)
      throw std::runtime_error(std::string("vgx_scan_registration_refine: ") + vgx_last_error(ctx_));
    for (int k = 0; k < 7; ++k) T_S_C_refined[k] = out[k];
    return summary_.usable != 0;
  }

  vgx_ctx ctx_;
  GpuTsdfLayer* layer_;
  vgx_scan_registration reg_ = nullptr;
  vgx_pose_graph_options options_;
  vgx_scan_registration_summary summary_{};
  double delta_[4] = {0.0, 0.0, 0.0, 0.0};
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_SCAN_TO_MAP_REGISTERER_H_
