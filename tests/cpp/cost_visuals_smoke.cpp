// The cost-function visuals of GpuRegistrationCostFunction (voxgraph_amd/cpp/gpu_registration_cost_function.h with
// gpu_cost_function_visuals.h) from plain C++ against the Ceres stub and the stand-in visualization_msgs/Marker.
//   cost_visuals_smoke compile    no device: the headers instantiate, the defaults and the marker constants
//   cost_visuals_smoke IN OUT     IN: one submap (voxel size, vps, blocks, four layers), its registration points with
//                                 weights, two poses.  A cost function with the three flags set and a recording sink is
//                                 evaluated once WITH and once WITHOUT Jacobians; a second one with the flags false
//                                 (same sink type) once.  OUT: per evaluation what the sink received.
// tests/test_cost_visuals_cpp.py compares OUT with the Python path and the restatement.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "gpu_registration_cost_function.h"
#include "marker_standin.h"

using voxgraph_amd::GpuRegistrationCostFunction;

struct RecordingSink : voxgraph_amd::CostFunctionVisualsSink {
  int transforms = 0, clouds = 0, markers = 0;
  voxgraph_amd::TransformView T;
  std::string T_frame, T_child;
  voxgraph_amd::ResidualCloudView cloud;
  std::string cloud_frame;
  std::vector<uint8_t> cloud_bytes;
  standin_marker::Marker arrows, origins;
  void OnTransform(const voxgraph_amd::TransformView& t) override {
    ++transforms;
    T = t;
    T_frame = t.frame_id;
    T_child = t.child_frame_id;
  }
  void OnResidualCloud(const voxgraph_amd::ResidualCloudView& c) override {
    ++clouds;
    cloud = c;
    cloud_frame = c.frame_id;
    cloud_bytes.assign(c.data, c.data + static_cast<size_t>(c.row_step) * c.height);
  }
  void OnJacobianMarkers(const voxgraph_amd::JacobianMarkersView& m) override {
    ++markers;
    voxgraph_amd::FillJacobianMarkers(m, &arrows, &origins);
  }
};

template <typename T>
static void get(std::ifstream& in, T* p, size_t n) {
  in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input file");
}

template <typename T>
static void put(std::ofstream& out, const T* p, size_t n) {
  out.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
}

static void put_string(std::ofstream& out, const std::string& s) {
  const int32_t n = static_cast<int32_t>(s.size());
  put(out, &n, 1);
  put(out, s.data(), s.size());
}

static int compile_checks() {
  GpuRegistrationCostFunction::Config cfg;
  if (cfg.visualize_residuals || cfg.visualize_gradients || cfg.visualize_transforms_) return 10;  // off as in the reference
  if (voxgraph_amd::kMarkerLineList != standin_marker::Marker::LINE_LIST || voxgraph_amd::kMarkerSphereList != 7 ||
      voxgraph_amd::kMarkerAdd != standin_marker::Marker::ADD)
    return 11;
  // the markers fill without a device
  const double arrow_points[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, origin_points[6] = {1, 2, 3, 7, 8, 9};
  voxgraph_amd::JacobianMarkersView view;
  view.arrow_points = arrow_points;
  view.origin_points = origin_points;
  view.n = 2;
  standin_marker::Marker arrows, origins;
  voxgraph_amd::FillJacobianMarkers(view, &arrows, &origins);
  if (arrows.points.size() != 4 || origins.points.size() != 2 || arrows.points[3].z != 12 || origins.points[1].x != 7) return 12;
  if (arrows.ns != "jacobian_vectors" || arrows.id != 1 || arrows.scale.x != 0.02 || arrows.color.r != 1.0f ||
      arrows.color.a != 1.0f || arrows.pose.orientation.w != 1.0 || arrows.header.frame_id != "mission")
    return 13;
  if (origins.ns != "jacobian_origins" || origins.id != 2 || origins.scale.x != 0.05 || origins.scale.y != 0.05 ||
      origins.scale.z != 0.05 || origins.color.r != 0.0f || origins.color.a != 1.0f || origins.frame_locked)
    return 14;
  const double pose[4] = {1.5, -2.0, 0.25, 0.0};
  const voxgraph_amd::TransformView T = voxgraph_amd::MissionReadingTransform(pose);
  if (T.q_wxyz[0] != 1.0f || T.q_wxyz[3] != 0.0f || T.t[0] != 1.5f || T.t[1] != -2.0f || T.t[2] != 0.25f) return 15;
  if (std::string(T.frame_id) != "mission" || std::string(T.child_frame_id) != "optimized_submap") return 16;
  RecordingSink sink;  // the sink interface instantiates
  auto ctor = [](vgx_ctx c, vgx_submap a, vgx_submap b, const GpuRegistrationCostFunction::Config& k,
                 voxgraph_amd::CostFunctionVisualsSink* s) { return new GpuRegistrationCostFunction(c, a, b, k, s); };
  (void)ctor;
  if (sink.clouds != 0) return 17;
  std::printf("COST_VISUALS_COMPILE_OK\n");
  return 0;
}

static void write_marker(std::ofstream& out, const standin_marker::Marker& m) {
  put_string(out, m.header.frame_id);
  put_string(out, m.ns);
  const int32_t head[4] = {m.id, m.type, m.action, static_cast<int32_t>(m.frame_locked)};
  put(out, head, 4);
  const double nums[7] = {m.scale.x, m.scale.y, m.scale.z, m.pose.orientation.x, m.pose.orientation.y, m.pose.orientation.z,
                          m.pose.orientation.w};
  put(out, nums, 7);
  const float rgba[4] = {m.color.r, m.color.g, m.color.b, m.color.a};
  put(out, rgba, 4);
  const int64_t n = static_cast<int64_t>(m.points.size());
  put(out, &n, 1);
  put(out, reinterpret_cast<const double*>(m.points.data()), 3 * m.points.size());
}

// what the sink received in one evaluation (counts since the last call), then the rows
static void write_evaluation(std::ofstream& out, RecordingSink* sink, bool ok, const std::vector<double>& r,
                             const std::vector<double>& je, bool with_jac) {
  const int32_t head[4] = {ok ? 1 : 0, sink->transforms, sink->clouds, sink->markers};
  put(out, head, 4);
  if (sink->transforms) {
    put(out, sink->T.q_wxyz, 4);
    put(out, sink->T.t, 3);
    put_string(out, sink->T_frame);
    put_string(out, sink->T_child);
  }
  if (sink->clouds) {
    const uint32_t geo[4] = {sink->cloud.width, sink->cloud.height, sink->cloud.point_step, sink->cloud.row_step};
    put(out, geo, 4);
    put_string(out, sink->cloud_frame);
    put(out, sink->cloud_bytes.data(), sink->cloud_bytes.size());
  }
  if (sink->markers) {
    write_marker(out, sink->arrows);
    write_marker(out, sink->origins);
  }
  put(out, r.data(), r.size());
  if (with_jac) put(out, je.data(), je.size());
  sink->transforms = sink->clouds = sink->markers = 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "compile") == 0) return compile_checks();
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t vps = 0, nb = 0, n = 0;
  float vs = 0;
  get(in, &vps, 1);
  get(in, &nb, 1);
  get(in, &n, 1);
  get(in, &vs, 1);
  const size_t vox = static_cast<size_t>(vps) * vps * vps * nb;
  std::vector<int32_t> bi(3 * static_cast<size_t>(nb));
  std::vector<float> td(vox), tw(vox), ed(vox);
  std::vector<uint8_t> eo(vox);
  std::vector<float> xyz(3 * static_cast<size_t>(n)), dist(n), w(n);
  double ref_pose[4], read_pose[4];
  get(in, bi.data(), bi.size());
  get(in, td.data(), vox);
  get(in, tw.data(), vox);
  get(in, ed.data(), vox);
  get(in, eo.data(), vox);
  get(in, xyz.data(), xyz.size());
  get(in, dist.data(), dist.size());
  get(in, w.data(), w.size());
  get(in, ref_pose, 4);
  get(in, read_pose, 4);
  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) {
    std::printf("no device: %s\n", vgx_last_error(nullptr));
    return 3;
  }
  int rc = 0;
  vgx_submap sm = nullptr;
  if (vgx_submap_create(ctx, 0, vs, vps, nb, bi.data(), td.data(), tw.data(), ed.data(), eo.data(), &sm) != VGX_OK ||
      vgx_submap_set_points(sm, VGX_POINTS_VOXELS, n, xyz.data(), dist.data(), w.data(), 0) != VGX_OK) {
    std::printf("submap: %s\n", vgx_last_error(ctx));
    rc = 4;
  }
  if (rc == 0) {
    std::ofstream out(argv[2], std::ios::binary);
    RecordingSink sink;
    GpuRegistrationCostFunction::Config cfg;
    cfg.registration_point_type = VGX_POINTS_VOXELS;
    std::vector<double> r(n), jo(4 * static_cast<size_t>(n)), je(4 * static_cast<size_t>(n));
    const double* params[2] = {ref_pose, read_pose};
    double* jacs[2] = {jo.data(), je.data()};
    {
      GpuRegistrationCostFunction::Config on = cfg;
      on.visualize_residuals = on.visualize_gradients = on.visualize_transforms_ = true;
      GpuRegistrationCostFunction cf(ctx, sm, sm, on, &sink);
      if (cf.num_residuals() != n) rc = 5;
      bool ok = cf.Evaluate(params, r.data(), jacs);
      write_evaluation(out, &sink, ok, r, je, true);
      ok = cf.Evaluate(params, r.data(), nullptr);
      write_evaluation(out, &sink, ok, r, je, false);
    }
    {
      GpuRegistrationCostFunction cf(ctx, sm, sm, cfg, &sink);  // the flags false: the sink is never called
      const bool ok = cf.Evaluate(params, r.data(), jacs);
      write_evaluation(out, &sink, ok, r, je, true);
    }
    if (!out) rc = 6;
  }
  if (sm) vgx_submap_destroy(sm);
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("COST_VISUALS_SMOKE_OK\n");
  return rc;
}
