// voxgraph_amd/cpp/gpu_pose_graph.h from plain C++: the edge covariances.
//   pose_graph_covariance_smoke compile   no device: the header instantiates, the two 6x6 fill helpers of
//                                         loop_closure_edge_server.cpp are exact, an unknown id is refused
//   pose_graph_covariance_smoke OUT       on the GPU: the ring of 8 submap nodes of pose_graph_smoke.cpp, solved, then
//                                         getEdgeCovarianceMap for six pairs (one with the constant submap, one (a, a),
//                                         one in both directions); an unknown id gives false.  OUT: the 8 poses, then
//                                         the six blocks in the map's order (f64).
// tests/test_pose_graph_covariance_cpp.py asks the Python wrapper for the same blocks and compares.
#include <cmath>
#include <cstdio>
#include <fstream>

#include "gpu_pose_graph.h"

using voxgraph_amd::GpuPoseGraph;

static const double kOdometryInformation[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2500, 0, 0, 0, 0, 2500};
static const double kLoopInformation[16] = {100, 20, 0, 0, 20, 100, 0, 0, 0, 0, 2500, 0, 0, 0, 0, 2500};

static int compile_checks() {
  double cov4[16], out[36];
  for (int i = 0; i < 16; ++i) cov4[i] = 1.0 + i;
  voxgraph_amd::FillLoopClosureEdgeCovariance(cov4, out);
  const int at[4] = {0, 1, 2, 5};
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) {
      double want = 1e4;
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
          if (at[i] == r && at[j] == c) want = cov4[4 * i + j];
      if (out[6 * r + c] != want) return 10;
    }
  voxgraph_amd::FillLoopClosureEdgeCovariance(cov4, out, -1.0);
  if (out[3] != -1.0 || out[6 * 4 + 4] != -1.0 || out[6 * 5 + 5] != 16.0 || out[5] != 4.0 || out[6 * 5] != 13.0) return 11;
  voxgraph_amd::IdentityLoopClosureEdgeCovariance(out);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c)
      if (out[6 * r + c] != (r == c ? 1.0 : 0.0)) return 12;
  GpuPoseGraph graph(nullptr);
  graph.addSubmapNode(7, {0, 0, 0, 0}, true);
  graph.addSubmapNode(9, {1, 0, 0, 0}, false);
  GpuPoseGraph::EdgeCovarianceMap map;
  if (!graph.getEdgeCovarianceMap(&map)) return 13;  // nothing asked: nothing computed
  map[{7, 8}] = {};
  if (graph.getEdgeCovarianceMap(&map) || graph.last_error().find("unknown submap") == std::string::npos) return 14;
  if (graph.getEdgeCovarianceMap(nullptr)) return 15;
  std::printf("POSE_GRAPH_COVARIANCE_COMPILE_OK\n");
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
    GpuPoseGraph::EdgeCovarianceMap map;
    for (const auto& pair : {std::pair<int64_t, int64_t>{101, 102}, {102, 101}, {103, 107}, {100, 104}, {105, 105}, {107, 101}}) map[pair] = {};
    if (rc == 0 && !graph.getEdgeCovarianceMap(&map)) {
      std::printf("getEdgeCovarianceMap: %s\n", graph.last_error().c_str());
      rc = 25;
    }
    if (rc == 0) {
      GpuPoseGraph::EdgeCovarianceMap unknown = map;
      unknown[{101, 999}] = {};
      if (graph.getEdgeCovarianceMap(&unknown)) rc = 26;
    }
    if (rc == 0) {
      std::ofstream out(argv[1], std::ios::binary);
      for (const auto& kv : graph.getSubmapPoses()) out.write(reinterpret_cast<const char*>(kv.second.data()), 4 * sizeof(double));
      for (const auto& kv : map) out.write(reinterpret_cast<const char*>(kv.second.data()), 16 * sizeof(double));
    }
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("POSE_GRAPH_COVARIANCE_SMOKE_OK\n");
  return rc;
}
