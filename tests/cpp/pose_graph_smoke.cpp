// voxgraph_amd/cpp/gpu_pose_graph.h from plain C++.
//   pose_graph_smoke compile   no device: the header instantiates, SqrtInformation is the LLT's L^T, nodes are numbered
//   pose_graph_smoke OUT       on the GPU: a ring of 8 submap nodes with drifting odometry, one loop closure and one
//                              absolute constraint from a reference-frame node (no registration constraints: they need
//                              submaps), solved; the error convention on a graph without constraints.  OUT: the
//                              summary's counts and costs, then the 8 poses (f64).
// tests/test_pose_graph_cpp.py solves the same graph through the Python wrapper and compares.
#include <cmath>
#include <cstdio>
#include <fstream>

#include "gpu_pose_graph.h"

using voxgraph_amd::GpuPoseGraph;

static const double kOdometryInformation[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2500, 0, 0, 0, 0, 2500};
// a full information matrix (correlated x / y)
static const double kLoopInformation[16] = {100, 20, 0, 0, 20, 100, 0, 0, 0, 0, 2500, 0, 0, 0, 0, 2500};

static int compile_checks() {
  double S[16];
  if (!voxgraph_amd::SqrtInformation(kLoopInformation, S)) return 10;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double v = 0;
      for (int k = 0; k < 4; ++k) v += S[4 * k + i] * S[4 * k + j];  // S^T S = information
      if (std::fabs(v - kLoopInformation[4 * i + j]) > 1e-9) return 11;
      if (i > j && S[4 * i + j] != 0.0) return 12;                   // upper triangular: L^T
    }
  const double bad[16] = {1, 2, 0, 0, 2, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (voxgraph_amd::SqrtInformation(bad, S)) return 13;
  GpuPoseGraph graph(nullptr);
  if (graph.options().parameter_tolerance != 3e-3 || graph.options().max_num_iterations != 50) return 14;
  if (graph.addSubmapNode(7, {0, 0, 0, 0}, true) != 0 || graph.addReferenceFrameNode(0, {0, 0, 0, 0}) != 1 ||
      graph.addSubmapNode(9, {1, 0, 0, 0}, false) != 2 || graph.addSubmapNode(7, {0.5, 0, 0, 0}, true) != 0)
    return 15;
  const double t[3] = {1, 0, 0};
  if (!graph.addRelativePoseConstraint(7, 9, t, 0.0, kOdometryInformation) || graph.addRelativePoseConstraint(7, 8, t, 0.0, kOdometryInformation) ||
      graph.addRelativePoseConstraint(7, 9, t, 0.0, bad) || graph.last_error().empty())
    return 16;
  if (graph.getSubmapPoses().size() != 2 || graph.getSubmapPoses()[7][0] != 0.5) return 17;
  std::printf("POSE_GRAPH_COMPILE_OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (std::string(argv[1]) == "compile") return compile_checks();
  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) {
    std::printf("no context: %s\n", vgx_last_error(nullptr));
    return 3;
  }
  int rc = 0;
  {
    GpuPoseGraph empty(ctx);
    empty.addSubmapNode(0, {0, 0, 0, 0}, true);
    empty.addSubmapNode(1, {1, 0, 0, 0}, false);
    if (empty.optimize() != VGX_ERR_INVALID || empty.last_error().find("without constraints") == std::string::npos) rc = 20;
  }
  {  // (the graph goes before its context does: its destructor synchronises the context's stream)
    GpuPoseGraph graph(ctx);
    const int n = 8;
    graph.addReferenceFrameNode(0, {0, 0, 0, 0});
    for (int k = 0; k < n; ++k) {
      const double a = 2.0 * M_PI * k / n;
      graph.addSubmapNode(100 + k, {2.0 * std::cos(a) - 2.0 + 0.05 * k, 2.0 * std::sin(a) - 0.03 * k, 0.01 * k, 0.9 * a / M_PI - 0.01 * k}, k == 0);
    }
    for (int k = 0; k + 1 < n; ++k) {
      const double a = 2.0 * M_PI * k / n, b = 2.0 * M_PI * (k + 1) / n;
      const double dx = 2.0 * (std::cos(b) - std::cos(a)), dy = 2.0 * (std::sin(b) - std::sin(a)), ya = 0.9 * a / M_PI;
      const double t[3] = {std::cos(ya) * dx + std::sin(ya) * dy, -std::sin(ya) * dx + std::cos(ya) * dy, 0.0};
      if (!graph.addRelativePoseConstraint(100 + k, 101 + k, t, 0.9 * (b - a) / M_PI, kOdometryInformation)) rc = 21;
    }
    {
      const double a = 2.0 * M_PI * (n - 1) / n, ya = 0.9 * a / M_PI;
      const double dx = 2.0 * (1.0 - std::cos(a)), dy = -2.0 * std::sin(a);
      const double t[3] = {std::cos(ya) * dx + std::sin(ya) * dy, -std::sin(ya) * dx + std::cos(ya) * dy, 0.0};
      if (!graph.addRelativePoseConstraint(100 + n - 1, 100, t, -ya, kLoopInformation)) rc = 22;
      const double height[3] = {-4.0, 0.0, 0.0};
      if (!graph.addAbsolutePoseConstraint(0, 100 + n / 2, height, 0.9, kOdometryInformation)) rc = 23;
    }
    if (rc == 0 && graph.optimize(false) != VGX_OK) {
      std::printf("optimize: %s\n", graph.last_error().c_str());
      rc = 24;
    }
    if (rc == 0) {
      const vgx_pose_graph_summary& s = graph.getSolverSummaries().back();
      if (s.termination_type != VGX_CONVERGENCE || !(s.final_cost < s.initial_cost) || graph.lastHistory().size() != static_cast<size_t>(s.num_iterations))
        rc = 25;
      std::ofstream out(argv[1], std::ios::binary);
      const double head[4] = {static_cast<double>(s.num_iterations), static_cast<double>(s.termination_reason), s.initial_cost, s.final_cost};
      out.write(reinterpret_cast<const char*>(head), sizeof(head));
      for (const auto& kv : graph.getSubmapPoses()) out.write(reinterpret_cast<const char*>(kv.second.data()), 4 * sizeof(double));
    }
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("POSE_GRAPH_SMOKE_OK\n");
  return rc;
}
