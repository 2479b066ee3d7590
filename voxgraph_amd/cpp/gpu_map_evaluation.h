// voxgraph::MapEvaluation::evaluate on the GPU.
//
// MapEvaluation (voxgraph/src/tools/evaluation/map_evaluation.cpp:59-114) scores the projected map of a submap collection
// against a ground-truth TSDF: projected map, finishSubmap() of both, alignSubmapAtoSubmapB (Ceres over one
// RegistrationCostFunction, :116-161), transformSubmap of the ground truth, evaluateLayersRmse of the two ESDF layers in
// kIgnoreErrorBehindTestSurface mode.  Every voxel loop of that runs on the device here; one details struct comes back
// (and the error layer, when asked for).  The swap inside map_evaluation.cpp:
//
//   voxgraph_amd::GpuMapEvaluation gpu_eval(ctx, gt_handle, voxel_size, voxels_per_side);
//   const auto result = gpu_eval.evaluate(submap_collection);   // {details, T_ground_truth__reading}
//
// gt_handle: the ground truth as a vgx_submap holding its raw TSDF layer (vgx_submap_create or vgx_map_file_load_submap),
// pose identity, as MapEvaluation loads it.  The collection's submaps go through GpuSubmapRegistry (their raw TSDF layers
// are kept: the projection reads them).  Semantics: vgx_tsdf_layer_transform_submap and vgx_evaluate_layers_rmse in
// include/voxgraph_amd.h.
#ifndef VOXGRAPH_AMD_CPP_GPU_MAP_EVALUATION_H_
#define VOXGRAPH_AMD_CPP_GPU_MAP_EVALUATION_H_

#include <ceres/ceres.h>

#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_fast_tsdf_integrator.h"
#include "gpu_projected_map.h"
#include "gpu_registration_cost_function.h"

namespace voxgraph_amd {

namespace map_evaluation_detail {
inline void check(vgx_ctx ctx, int rc, const char* what) {
  if (rc != VGX_OK) throw std::runtime_error(std::string(what) + ": " + vgx_last_error(ctx));
}
// a vgx_submap owned for the length of a scope
struct OwnedSubmap {
  vgx_submap h = nullptr;
  OwnedSubmap() = default;
  OwnedSubmap(const OwnedSubmap&) = delete;
  OwnedSubmap& operator=(const OwnedSubmap&) = delete;
  ~OwnedSubmap() {
    if (h) vgx_submap_destroy(h);
  }
};
}  // namespace map_evaluation_detail

// VoxgraphSubmap::transformSubmap(T_new_old) on the device: the submap's raw TSDF layer resampled into a new frame
// (vgx_tsdf_layer_transform_submap), handed to a new submap and its ESDF regenerated (finishSubmap()).  The caller owns the
// returned handle.
inline vgx_submap TransformSubmapOnGpu(vgx_ctx ctx, vgx_submap submap, const float T_new_old[7], float voxel_size,
                                       int voxels_per_side, int32_t new_id) {
  GpuTsdfLayer layer(ctx, voxel_size, voxels_per_side);
  map_evaluation_detail::check(ctx, vgx_tsdf_layer_transform_submap(layer.handle(), submap, T_new_old, nullptr),
                               "vgx_tsdf_layer_transform_submap");
  vgx_submap out = nullptr;
  map_evaluation_detail::check(ctx, vgx_submap_from_tsdf_layer(ctx, layer.handle(), new_id, &out), "vgx_submap_from_tsdf_layer");
  const int rc = vgx_submap_generate_esdf(out, nullptr, nullptr);
  if (rc != VGX_OK) {
    const std::string msg = vgx_last_error(ctx);
    vgx_submap_destroy(out);
    throw std::runtime_error("vgx_submap_generate_esdf: " + msg);
  }
  return out;
}

// voxblox::utils::evaluateLayersRmse(gt, test, mode, &details, &error_layer) over two finished submaps' ESDF
// (VGX_EVAL_LAYER_ESDF) or TSDF layers.  The error layer (nullable vectors): one block per test block with a gt
// counterpart -- block_index [m][3], distance and set [m][vps^3].
struct GpuErrorLayer {
  std::vector<int32_t> block_index;
  std::vector<float> distance;
  std::vector<uint8_t> set;
};
inline vgx_voxel_evaluation_details EvaluateLayersRmseOnGpu(vgx_ctx ctx, vgx_submap gt, vgx_submap test, int32_t layer,
                                                            int32_t mode, int voxels_per_side,
                                                            GpuErrorLayer* error_layer = nullptr) {
  vgx_voxel_evaluation_details details{};
  if (!error_layer) {
    map_evaluation_detail::check(ctx, vgx_evaluate_layers_rmse(gt, test, layer, mode, &details, nullptr, nullptr, nullptr, nullptr),
                                 "vgx_evaluate_layers_rmse");
    return details;
  }
  const size_t n = static_cast<size_t>(vgx_submap_num_blocks(test));
  const size_t vox = static_cast<size_t>(voxels_per_side) * voxels_per_side * voxels_per_side;
  error_layer->block_index.resize(3 * n);
  error_layer->distance.resize(vox * n);
  error_layer->set.resize(vox * n);
  int32_t m = 0;
  map_evaluation_detail::check(ctx,
                               vgx_evaluate_layers_rmse(gt, test, layer, mode, &details, error_layer->block_index.data(),
                                                        error_layer->distance.data(), error_layer->set.data(), &m),
                               "vgx_evaluate_layers_rmse");
  error_layer->block_index.resize(3 * static_cast<size_t>(m));
  error_layer->distance.resize(vox * m);
  error_layer->set.resize(vox * m);
  return details;
}

class GpuMapEvaluation {
 public:
  struct EvaluationDetails {  // MapEvaluation::EvaluationDetails
    vgx_voxel_evaluation_details details;
    double T_ground_truth__reading[7];  // {qw,qx,qy,qz, tx,ty,tz}
    double aligned_pose[4];             // the ground truth's {x, y, z, yaw} in the projected map's frame
    int solver_iterations;
  };

  // ground_truth: see the file comment; the handle stays the caller's
  GpuMapEvaluation(vgx_ctx ctx, vgx_submap ground_truth, float voxel_size, int voxels_per_side)
      : ctx_(ctx), ground_truth_(ground_truth), voxel_size_(voxel_size), vps_(voxels_per_side) {}

  // error_cloud (with its config; gpu_layer_pointcloud.h): the evaluation goes through vgx_evaluate_layers_rmse_cloud and
  // the handle receives the point-cloud view of the error layer, which then never leaves the device -- the same details
  // bit for bit.  An alternative to error_layer, not an addition to it.
  template <typename CollectionT>
  EvaluationDetails evaluate(const CollectionT& collection, GpuErrorLayer* error_layer = nullptr,
                             const vgx_cloud_config* error_cloud_config = nullptr, vgx_cloud error_cloud = nullptr) const {
    using map_evaluation_detail::check;
    // the projected map, as a submap (map_evaluation.cpp:72-76)
    map_evaluation_detail::OwnedSubmap projected;
    {
      GpuTsdfLayer layer(ctx_, voxel_size_, vps_);
      GetProjectedMapOnGpu(collection, &layer);
      check(ctx_, vgx_submap_from_tsdf_layer(ctx_, layer.handle(), 1, &projected.h), "vgx_submap_from_tsdf_layer");
    }
    // finishSubmap() of both (:80-81): ESDF and the kVoxels points (VoxgraphSubmap::Config registration_filter defaults)
    for (vgx_submap sm : {projected.h, ground_truth_}) {
      check(ctx_, vgx_submap_generate_esdf(sm, nullptr, nullptr), "vgx_submap_generate_esdf");
      check(ctx_, vgx_submap_extract_voxel_points(sm, 1.0, 0.3, 1, nullptr), "vgx_submap_extract_voxel_points");
    }
    // alignSubmapAtoSubmapB(ground truth, projected map) (:116-161)
    EvaluationDetails out{};
    double layer_B_pose[4] = {0, 0, 0, 0};
    double layer_A_pose[4] = {0, 0, 0, 0};
    {
      ceres::Problem problem;
      ceres::Solver::Options options;
      options.max_num_iterations = 200;
      options.parameter_tolerance = 1e-12;
      GpuRegistrationCostFunction::Config cost_config;
      cost_config.use_esdf_distance = true;
      cost_config.sampling_ratio = -1;
      cost_config.registration_point_type = VGX_POINTS_VOXELS;
      problem.AddParameterBlock(layer_B_pose, 4);
      problem.SetParameterBlockConstant(layer_B_pose);
      problem.AddParameterBlock(layer_A_pose, 4);
      problem.AddResidualBlock(new GpuRegistrationCostFunction(ctx_, projected.h, ground_truth_, cost_config), nullptr,
                               layer_B_pose, layer_A_pose);
      ceres::Solver::Summary summary;
      ceres::Solve(options, &problem, &summary);
      out.solver_iterations = summary.num_iterations;
    }
    // T = Transformation::exp(x, y, z, 0, 0, yaw): minkindr's decoupled exp -- the translation as it is, a rotation
    // about z -- formed in f64 and rounded to f32 (voxblox::Transformation), as capi.map_evaluation does
    const double half = 0.5 * layer_A_pose[3];
    const float T[7] = {static_cast<float>(std::cos(half)), 0.0f, 0.0f, static_cast<float>(std::sin(half)),
                        static_cast<float>(layer_A_pose[0]), static_cast<float>(layer_A_pose[1]),
                        static_cast<float>(layer_A_pose[2])};
    for (int k = 0; k < 4; ++k) out.aligned_pose[k] = layer_A_pose[k];
    // transformSubmap(T) (:86), then evaluateLayersRmse(gt ESDF, projected ESDF, kIgnoreErrorBehindTestSurface) (:90-95)
    map_evaluation_detail::OwnedSubmap transformed;
    transformed.h = TransformSubmapOnGpu(ctx_, ground_truth_, T, voxel_size_, vps_, vgx_submap_id(ground_truth_));
    if (error_cloud) {
      if (error_layer) throw std::invalid_argument("GpuMapEvaluation::evaluate: error_layer and error_cloud are alternatives");
      check(ctx_,
            vgx_evaluate_layers_rmse_cloud(transformed.h, projected.h, VGX_EVAL_LAYER_ESDF, VGX_EVAL_IGNORE_BEHIND_TEST,
                                           &out.details, error_cloud_config, error_cloud),
            "vgx_evaluate_layers_rmse_cloud");
    } else {
      out.details = EvaluateLayersRmseOnGpu(ctx_, transformed.h, projected.h, VGX_EVAL_LAYER_ESDF, VGX_EVAL_IGNORE_BEHIND_TEST,
                                            vps_, error_layer);
    }
    // T_projected_map__ground_truth.inverse(): rotation about -yaw, translation -(R^-1 t)
    const double c = std::cos(layer_A_pose[3]), s = std::sin(layer_A_pose[3]);
    const double tx = layer_A_pose[0], ty = layer_A_pose[1], tz = layer_A_pose[2];
    const double inv[7] = {std::cos(0.5 * layer_A_pose[3]), 0.0, 0.0, -std::sin(0.5 * layer_A_pose[3]),
                           -(c * tx + s * ty), -(-s * tx + c * ty), -tz};
    for (int k = 0; k < 7; ++k) out.T_ground_truth__reading[k] = inv[k];
    return out;
  }

 private:
  vgx_ctx ctx_;
  vgx_submap ground_truth_;
  float voxel_size_;
  int vps_;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_MAP_EVALUATION_H_
