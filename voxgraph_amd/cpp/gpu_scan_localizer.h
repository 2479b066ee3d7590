// Scan localisation for the mapper: where is the sensor in the map that is already finished?  A scan's points against
// the ESDF (or TSDF) of posed, finished submaps -- many hypotheses scored in one call, the best one refined.  NOT a mirror
// of a reference class: the reference takes loop closures from outside and never verifies them; the formulation is the
// library's own (include/voxgraph_amd.h, "Scan localisation").  Plain structs, no ROS and no Eigen.  It
// stands beside GpuScanToMapRegisterer, which tracks against the ACTIVE layer:
//
//   localizer.setMap(GpuScanLocalizer::defaultMapConfig(), finished_submaps, T_M_S);   // after a solve: the optimised poses
//   localizer.setScan(integrator.scan());
//   auto r = localizer.localize(makeHypothesisGrid(grid));                 // re-localisation, or the start in a loaded map
//   bool ok = localizer.refine(T_M_C_proposed, T_M_C);                     // the check of one proposed loop closure
//
// Runs on the context's registration stream, behind vgx_submap_generate_esdf.
#ifndef VOXGRAPH_AMD_CPP_GPU_SCAN_LOCALIZER_H_
#define VOXGRAPH_AMD_CPP_GPU_SCAN_LOCALIZER_H_

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "voxgraph_amd.h"

namespace voxgraph_amd {

// Hypotheses on a horizontal grid: x_min + i step <= x_max, y_min + j step <= y_max (a hair of slack for the last one),
// n_yaw headings 2 pi k / n_yaw about the mission z axis applied ON TOP of q_prior, whose roll and pitch (and heading)
// every hypothesis keeps: q = q_z(yaw_k) (x) q_prior, formed in f64 and rounded once.  z is fixed.
struct HypothesisGrid {
  double x_min = 0, x_max = 0, y_min = 0, y_max = 0, step = 1;
  int32_t n_yaw = 1;
  double z = 0;
  float q_prior[4] = {1.0f, 0.0f, 0.0f, 0.0f};
};

// -> poses [n][7] {qw,qx,qy,qz, tx,ty,tz}, x-major, then y, then yaw
inline std::vector<float> makeHypothesisGrid(const HypothesisGrid& g) {
  if (!(g.step > 0.0) || g.n_yaw < 1) throw std::invalid_argument("makeHypothesisGrid: step <= 0 or n_yaw < 1");
  std::vector<float> poses;
  const double slack = 1e-9 * g.step;
  const double w = g.q_prior[0], qx = g.q_prior[1], qy = g.q_prior[2], qz = g.q_prior[3];
  for (int i = 0; g.x_min + i * g.step <= g.x_max + slack; ++i)
    for (int j = 0; g.y_min + j * g.step <= g.y_max + slack; ++j)
      for (int k = 0; k < g.n_yaw; ++k) {
        const double yaw = 2.0 * M_PI * k / g.n_yaw;
        const double cz = std::cos(0.5 * yaw), sz = std::sin(0.5 * yaw);
        const float T[7] = {(float)(cz * w - sz * qz),       (float)(cz * qx - sz * qy),      (float)(cz * qy + sz * qx),
                            (float)(cz * qz + sz * w),       (float)(g.x_min + i * g.step),   (float)(g.y_min + j * g.step),
                            (float)g.z};
        poses.insert(poses.end(), T, T + 7);
      }
  return poses;
}

struct ScanLocalizerResult {
  int32_t best_index = -1;  // the hypothesis refined; -1: none had enough usable points
  bool usable = false;
  float T_M_C[7] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // refined when usable, else the hypothesis' own bits
  double delta[4] = {0.0, 0.0, 0.0, 0.0};
  vgx_scan_registration_summary summary{};
};

struct ScanPoseScores {
  std::vector<double> cost;
  std::vector<int64_t> n_terms, n_points_valid, n_candidates;
};

class GpuScanLocalizer {
 public:
  using Config = vgx_scan_registration_config;
  using MapConfig = vgx_scan_map_config;
  static Config defaultConfig(float max_abs_distance_m) {
    Config c;
    vgx_scan_registration_config_default(&c);
    c.max_abs_distance_m = max_abs_distance_m;
    return c;
  }
  static MapConfig defaultMapConfig() {
    MapConfig c;
    vgx_scan_map_config_default(&c);
    return c;
  }

  GpuScanLocalizer(vgx_ctx ctx, const Config& config) : ctx_(ctx) {
    vgx_pose_graph_options_default(&options_);
    check(vgx_scan_registration_create(ctx, &config, &reg_), "vgx_scan_registration_create");
  }
  ~GpuScanLocalizer() { vgx_scan_registration_destroy(reg_); }
  GpuScanLocalizer(const GpuScanLocalizer&) = delete;
  GpuScanLocalizer& operator=(const GpuScanLocalizer&) = delete;
  vgx_scan_registration handle() const { return reg_; }
  void setSolverOptions(const vgx_pose_graph_options& options) { options_ = options; }

  // finished submaps and their poses T_M_S [n][7]; the handle keeps the submaps alive until the next setMap
  void setMap(const MapConfig& config, const std::vector<vgx_submap>& submaps, const std::vector<float>& T_M_S) {
    if (T_M_S.size() != 7 * submaps.size()) throw std::invalid_argument("setMap: one pose per submap");
    check(vgx_scan_registration_set_map(reg_, &config, (int32_t)submaps.size(), submaps.data(), T_M_S.data()),
          "vgx_scan_registration_set_map");
  }
  void clearMap() { check(vgx_scan_registration_set_map(reg_, nullptr, 0, nullptr, nullptr), "vgx_scan_registration_set_map"); }

  // the scan: a decoded vgx_scan (borrowed), host points [n][3] f32 (copied), or device points ready with respect to the
  // registration stream (borrowed)
  void setScan(vgx_scan scan) { check(vgx_scan_registration_set_scan(reg_, scan), "vgx_scan_registration_set_scan"); }
  void setPoints(const float* points_C, int64_t n) { check(vgx_scan_registration_set_points(reg_, points_C, n), "vgx_scan_registration_set_points"); }
  void setPointsDevice(const void* d_points_C, int64_t n) {
    check(vgx_scan_registration_set_points_device(reg_, d_points_C, n), "vgx_scan_registration_set_points_device");
  }

  ScanPoseScores scorePoses(const std::vector<float>& T_M_C) {
    const size_t n = T_M_C.size() / 7;
    ScanPoseScores s;
    s.cost.resize(n);
    s.n_terms.resize(n);
    s.n_points_valid.resize(n);
    s.n_candidates.resize(n);
    check(vgx_scan_registration_score_poses(reg_, (int32_t)n, T_M_C.data(), s.cost.data(), s.n_terms.data(), s.n_points_valid.data(),
                                            s.n_candidates.data()),
          "vgx_scan_registration_score_poses");
    return s;
  }

  // one proposed pose (a loop-closure candidate): returns `usable`; T_M_C_refined is the prior's bits otherwise
  bool refine(const float T_M_C_prior[7], float T_M_C_refined[7]) {
    float out[7];
    check(vgx_scan_registration_refine_map(reg_, T_M_C_prior, &options_, out, delta_, &summary_), "vgx_scan_registration_refine_map");
    for (int k = 0; k < 7; ++k) T_M_C_refined[k] = out[k];
    return summary_.usable != 0;
  }

  ScanLocalizerResult localize(const std::vector<float>& T_M_C) {
    ScanLocalizerResult r;
    check(vgx_scan_registration_localize(reg_, (int32_t)(T_M_C.size() / 7), T_M_C.data(), &options_, &r.best_index, r.T_M_C, r.delta,
                                         &r.summary),
          "vgx_scan_registration_localize");
    r.usable = r.summary.usable != 0;
    summary_ = r.summary;
    for (int k = 0; k < 4; ++k) delta_[k] = r.delta[k];
    return r;
  }

  const vgx_scan_registration_summary& lastSummary() const { return summary_; }
  const double* lastCorrection() const { return delta_; }

 private:
  void check(int rc, const char* what) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string(what) + ": " + (ctx_ ? vgx_last_error(ctx_) : "no context"));
  }

  vgx_ctx ctx_;
  vgx_scan_registration reg_ = nullptr;
  vgx_pose_graph_options options_;
  vgx_scan_registration_summary summary_{};
  double delta_[4] = {0.0, 0.0, 0.0, 0.0};
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_SCAN_LOCALIZER_H_
