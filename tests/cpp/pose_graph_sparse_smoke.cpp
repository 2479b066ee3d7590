// GpuPoseGraph::setLinearSolver (voxgraph_amd/cpp/gpu_pose_graph.h) from plain C++.
//   pose_graph_sparse_smoke compile   no device: the header instantiates; a permutation of the wrong length is refused
//                                     before any library call
//   pose_graph_sparse_smoke run       on the GPU: a drifting chain of 40 submap nodes with second-neighbour edges and one
//                                     loop closure (nf = 156: three panels), solved with the dense solver, the
//                                     tile-sparse one in natural order (the same poses, value for value) and under RCM
//                                     (within 1e-6 of them); the structure's counts.
#include <cmath>
#include <cstdio>
#include <string>

#include "gpu_pose_graph.h"

using voxgraph_amd::GpuPoseGraph;

static const double kOdometryInformation[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 2500, 0, 0, 0, 0, 2500};
static const double kLoopInformation[16] = {100, 20, 0, 0, 20, 100, 0, 0, 0, 0, 2500, 0, 0, 0, 0, 2500};
static const int kNodes = 40;

static void true_pose(int k, double p[4]) {
  const double a = 0.15 * k;
  p[0] = 3.0 * std::cos(a) - 3.0, p[1] = 3.0 * std::sin(a), p[2] = 0.02 * k, p[3] = 0.5 * a;
}
static bool add_edge(GpuPoseGraph& g, int a, int b, const double* information) {
  double pa[4], pb[4];
  true_pose(a, pa), true_pose(b, pb);
  const double c = std::cos(pa[3]), s = std::sin(pa[3]), dx = pb[0] - pa[0], dy = pb[1] - pa[1];
  const double t[3] = {c * dx + s * dy + 0.01 * ((a * 7 + b) % 5 - 2), -s * dx + c * dy - 0.01 * ((a + 3 * b) % 3 - 1), pb[2] - pa[2]};
  return g.addRelativePoseConstraint(a, b, t, pb[3] - pa[3] + 0.002 * ((a + b) % 3 - 1), information);
}
static bool fill(GpuPoseGraph& g) {
  bool ok = true;
  for (int k = 0; k < kNodes; ++k) {
    double p[4];
    true_pose(k, p);
    g.addSubmapNode(k, {p[0] + 0.02 * k, p[1] - 0.015 * k, p[2] + 0.001 * k, p[3] + 0.003 * k}, k == 0);
  }
  for (int k = 0; k + 1 < kNodes; ++k) ok = ok && add_edge(g, k, k + 1, kOdometryInformation);
  for (int k = 0; k + 2 < kNodes; ++k) ok = ok && add_edge(g, k, k + 2, kOdometryInformation);
  return ok && add_edge(g, kNodes - 2, 3, kLoopInformation);
}

static int compile_checks() {
  GpuPoseGraph graph(nullptr);
  if (!fill(graph)) return 10;
  if (graph.setLinearSolver(VGX_LINEAR_SOLVER_TILE_SPARSE, VGX_ORDER_GIVEN, {0, 1, 2}) != VGX_OK) return 9;  // kept for optimize()
  if (graph.optimize() != VGX_ERR_INVALID || graph.last_error().find("permutation") == std::string::npos) return 11;
  vgx_pose_graph_structure_stats stats;
  if (graph.getStructure(&stats)) return 12;
  int32_t order[4] = {0}, tiles[8] = {0}, n_tiles = 0;
  const int32_t pairs[4] = {1, 0, 3, 2};
  if (vgx_pose_graph_tile_pattern(4, 2, pairs, VGX_ORDER_NATURAL, nullptr, order, 4, tiles, &n_tiles) != VGX_OK || n_tiles != 1 || order[3] != 3)
    return 13;
  std::printf("POSE_GRAPH_SPARSE_COMPILE_OK\n");
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
    GpuPoseGraph dense(ctx), sparse(ctx), rcm(ctx);
    if (!fill(dense) || !fill(sparse) || !fill(rcm)) rc = 20;
    sparse.setLinearSolver(VGX_LINEAR_SOLVER_TILE_SPARSE);
    rcm.setLinearSolver(VGX_LINEAR_SOLVER_TILE_SPARSE, VGX_ORDER_RCM);
    for (GpuPoseGraph* g : {&dense, &sparse, &rcm})
      if (rc == 0 && g->optimize() != VGX_OK) {
        std::printf("optimize: %s\n", g->last_error().c_str());
        rc = 21;
      }
    if (rc == 0) {
      const vgx_pose_graph_summary &sd = dense.getSolverSummaries().back(), &ss = sparse.getSolverSummaries().back();
      if (sd.termination_type != VGX_CONVERGENCE || !(sd.final_cost < sd.initial_cost) || sd.num_successful_steps < 1) rc = 22;
      if (ss.num_iterations != sd.num_iterations || ss.final_cost != sd.final_cost || ss.initial_cost != sd.initial_cost) rc = 23;
      const auto pd = dense.getSubmapPoses(), ps = sparse.getSubmapPoses(), pr = rcm.getSubmapPoses();
      double worst = 0.0;
      for (int k = 0; k < kNodes && rc == 0; ++k)
        for (int c = 0; c < 4; ++c) {
          if (ps.at(k)[c] != pd.at(k)[c]) rc = 24;
          worst = std::fmax(worst, std::fabs(pr.at(k)[c] - pd.at(k)[c]));
        }
      if (rc == 0 && !(worst < 1e-6)) rc = 25;
      vgx_pose_graph_structure_stats stats;
      if (rc == 0 && (dense.getStructure(&stats) || !sparse.getStructure(&stats))) rc = 26;
      // on the live handle: a refused setting changes nothing, a taken one shows in the next solve
      if (rc == 0 && (dense.setLinearSolver(5) != VGX_ERR_INVALID || dense.setLinearSolver(VGX_LINEAR_SOLVER_TILE_SPARSE, VGX_ORDER_GIVEN, {1, 2}) != VGX_ERR_INVALID))
        rc = 28;
      if (rc == 0 && (dense.optimize() != VGX_OK || dense.getStructure(&stats))) rc = 29;
      if (rc == 0 && (dense.setLinearSolver(VGX_LINEAR_SOLVER_TILE_SPARSE) != VGX_OK || dense.optimize() != VGX_OK || !dense.getStructure(&stats))) rc = 30;
      // 39 free nodes: three tile rows; the chain joins neighbouring tiles, the closure (38, 3) tiles 2 and 0
      if (rc == 0 && (stats.n_free_variables != 156 || stats.n_panels != 3 || stats.n_l_tiles != 6 || stats.n_h_tiles != 9 ||
                      stats.n_update_triples != 4 || stats.n_launches != 7))
        rc = 27;
      std::printf("dense / sparse / rcm: %d iterations, final cost %.17g, rcm off by %.3e\n", sd.num_iterations, sd.final_cost, worst);
    }
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("POSE_GRAPH_SPARSE_SMOKE_OK\n");
  return rc;
}
