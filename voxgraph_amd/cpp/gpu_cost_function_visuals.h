// Cost-function visuals of the GPU registration cost function: what voxgraph::CostFunctionVisuals publishes while
// RegistrationCostFunction::Evaluate runs (voxgraph/src/tools/visualization/cost_function_visuals.cpp, cited as CFV;
// registration_cost_function.cpp:102-106, 169-176, 244-252, 293-295, cited as RCF) -- the residual cloud, the two
// Jacobian markers and the TF of the reading submap's pose -- handed to a sink instead of to ROS publishers.  The arrays
// are made on the device by vgx_reg_evaluate_visuals (include/voxgraph_amd.h, "Cost-function visuals"); the fixed
// marker fields (CFV:13-40) are the constants below.  No ROS type is named here: FillJacobianMarkers is a template over
// the marker type (visualization_msgs::Marker, or the stand-in of tests/cpp/marker_standin.h).
#ifndef VOXGRAPH_AMD_CPP_GPU_COST_FUNCTION_VISUALS_H_
#define VOXGRAPH_AMD_CPP_GPU_COST_FUNCTION_VISUALS_H_

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "voxgraph_amd.h"

namespace voxgraph_amd {

constexpr const char* kVisualsFrame = "mission";                // CFV:13, 18; RCF:104
constexpr const char* kVisualsChildFrame = "optimized_submap";  // RCF:105
constexpr int32_t kMarkerLineList = 5;    // visualization_msgs::Marker::LINE_LIST
constexpr int32_t kMarkerSphereList = 7;  // visualization_msgs::Marker::SPHERE_LIST
constexpr int32_t kMarkerAdd = 0;         // visualization_msgs::Marker::ADD

// pcl::PointCloud<pcl::PointXYZI> as the bytes of a sensor_msgs/PointCloud2 body: `width` records of point_step bytes
// (x y z f32 at 0 4 8, 1.0f at 12, intensity f32 at 16, zero padding), height 1, dense
struct ResidualCloudView {
  const uint8_t* data = nullptr;
  uint32_t width = 0, height = 1, point_step = 32, row_step = 0;
  const char* frame_id = kVisualsFrame;
};

// marker.points of the two Jacobian markers (geometry_msgs/Point = three f64)
struct JacobianMarkersView {
  const double* arrow_points = nullptr;   // [2 n][3]: origin 0, tip 0, origin 1, tip 1, ..  (LINE_LIST)
  const double* origin_points = nullptr;  // [n][3]                                           (SPHERE_LIST)
  size_t n = 0;
};

// T_mission__reading (RCF:80-88): minkindr's exp of the reading pose narrowed to f32
struct TransformView {
  float q_wxyz[4] = {1, 0, 0, 0};
  float t[3] = {0, 0, 0};
  const char* frame_id = kVisualsFrame;
  const char* child_frame_id = kVisualsChildFrame;
};

// Receives the visuals after each Evaluate that returned true (RCF:293-295: nothing is published when it returns
// false; an empty cloud or empty markers are not published either, CFV:93-100).  Called on the evaluating thread; the
// views are valid during the call only.
class CostFunctionVisualsSink {
 public:
  virtual ~CostFunctionVisualsSink() = default;
  virtual void OnTransform(const TransformView&) {}                // visualize_transforms_, before the evaluation
  virtual void OnResidualCloud(const ResidualCloudView&) {}        // visualize_residuals
  virtual void OnJacobianMarkers(const JacobianMarkersView&) {}    // visualize_gradients, Jacobians asked for
};

inline TransformView MissionReadingTransform(const double read_pose[4]) {
  TransformView T;
  // RotationQuaternionTemplate<float>::exp for (0, 0, yaw): double internals, narrowed to float
  const float psi = static_cast<float>(read_pose[3]);
  const float nrm = std::sqrt(0.0f * 0.0f + 0.0f * 0.0f + psi * psi);
  const double theta = static_cast<double>(nrm);
  const double na = theta < std::pow(2.220446049250313e-16, 0.25) ? 0.5 + (theta * theta) * (1.0 / 48.0)
                                                                  : std::sin(theta * 0.5) / theta;
  T.q_wxyz[0] = static_cast<float>(std::cos(theta * 0.5));
  T.q_wxyz[1] = 0.0f;
  T.q_wxyz[2] = 0.0f;
  T.q_wxyz[3] = static_cast<float>(static_cast<double>(psi) * na);
  for (int a = 0; a < 3; ++a) T.t[a] = static_cast<float>(read_pose[a]);
  return T;
}

// The two markers of CFV:13-40 with the points of `view`: header.frame_id, ns, id, type, action, pose.orientation.w,
// scale, color and frame_locked are written; header.stamp is the caller's (the reference stamps them once, at
// construction).
template <typename Marker>
void FillJacobianMarkers(const JacobianMarkersView& view, Marker* arrows, Marker* origins) {
  arrows->header.frame_id = kVisualsFrame;
  arrows->ns = "jacobian_vectors";
  arrows->id = 1;
  arrows->type = kMarkerLineList;
  arrows->action = kMarkerAdd;
  arrows->pose.orientation.w = 1.0;
  arrows->scale.x = 0.02;
  arrows->color.r = 1.0f;  // voxblox::Color::Red()
  arrows->color.g = 0.0f;
  arrows->color.b = 0.0f;
  arrows->color.a = 1.0f;
  arrows->frame_locked = false;
  origins->header.frame_id = kVisualsFrame;
  origins->ns = "jacobian_origins";
  origins->id = 2;
  origins->type = kMarkerSphereList;
  origins->action = kMarkerAdd;
  origins->pose.orientation.w = 1.0;
  origins->scale.x = 0.05;
  origins->scale.y = 0.05;
  origins->scale.z = 0.05;
  origins->color.r = 0.0f;  // voxblox::Color::Black()
  origins->color.g = 0.0f;
  origins->color.b = 0.0f;
  origins->color.a = 1.0f;
  origins->frame_locked = false;
  arrows->points.resize(2 * view.n);
  origins->points.resize(view.n);
  for (size_t i = 0; i < 2 * view.n; ++i) {
    arrows->points[i].x = view.arrow_points[3 * i];
    arrows->points[i].y = view.arrow_points[3 * i + 1];
    arrows->points[i].z = view.arrow_points[3 * i + 2];
  }
  for (size_t i = 0; i < view.n; ++i) {
    origins->points[i].x = view.origin_points[3 * i];
    origins->points[i].y = view.origin_points[3 * i + 1];
    origins->points[i].z = view.origin_points[3 * i + 2];
  }
}

// The device handle and the host staging of one cost function's visuals (reused from Evaluate to Evaluate)
class GpuCostFunctionVisuals {
 public:
  explicit GpuCostFunctionVisuals(vgx_ctx ctx) : ctx_(ctx) {
    if (vgx_reg_visuals_create(ctx, &handle_) != VGX_OK)
      throw std::runtime_error(std::string("vgx_reg_visuals_create: ") + vgx_last_error(ctx));
  }
  ~GpuCostFunctionVisuals() { vgx_reg_visuals_destroy(handle_); }
  GpuCostFunctionVisuals(const GpuCostFunctionVisuals&) = delete;
  GpuCostFunctionVisuals& operator=(const GpuCostFunctionVisuals&) = delete;

  vgx_reg_visuals handle() const { return handle_; }

  // downloads what the handle holds and hands it to the sink
  void Publish(CostFunctionVisualsSink* sink) {
    int64_t n_cloud = 0, n_jac = 0;
    if (vgx_reg_visuals_stats(handle_, &n_cloud, &n_jac) != VGX_OK) throw std::runtime_error("vgx_reg_visuals_stats");
    cloud_.resize(static_cast<size_t>(n_cloud) * 32);
    arrows_.resize(static_cast<size_t>(n_jac) * 6);
    origins_.resize(static_cast<size_t>(n_jac) * 3);
    if (vgx_reg_visuals_download(handle_, cloud_.data(), arrows_.data(), origins_.data(), nullptr) != VGX_OK)
      throw std::runtime_error(std::string("vgx_reg_visuals_download: ") + vgx_last_error(ctx_));
    if (n_cloud != 0) {  // CFV:93-95
      ResidualCloudView c;
      c.data = cloud_.data();
      c.width = static_cast<uint32_t>(n_cloud);
      c.row_step = c.width * c.point_step;
      sink->OnResidualCloud(c);
    }
    if (n_jac != 0) {  // CFV:96-100
      JacobianMarkersView m;
      m.arrow_points = arrows_.data();
      m.origin_points = origins_.data();
      m.n = static_cast<size_t>(n_jac);
      sink->OnJacobianMarkers(m);
    }
  }

 private:
  vgx_ctx ctx_;
  vgx_reg_visuals handle_ = nullptr;
  std::vector<uint8_t> cloud_;
  std::vector<double> arrows_, origins_;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_COST_FUNCTION_VISUALS_H_
