// A host mirror of voxgraph::PoseGraph (voxgraph/include/voxgraph/backend/pose_graph.h) as far as solving goes, on
// vgx_pose_graph (include/voxgraph_amd.h, "Pose graph: the solve"): nodes, registration / relative / absolute pose
// constraints, optimize(), getSubmapPoses(), getEdgeCovarianceMap() and the stored summaries.  No Ceres, no Eigen.
//
//   voxgraph_amd::GpuPoseGraph graph(gpu_ctx);
//   graph.addSubmapNode(id, pose, /*constant=*/id == first);            // pose_graph_interface.cpp:24-48
//   graph.addRegistrationConstraint(reg_first_second, first, second);   // registration_constraint.cpp:33-42
//   graph.addRelativePoseConstraint(a, b, t_ab, yaw_ab, information);   // odometry, loop closures
//   graph.addAbsolutePoseConstraint(frame, id, t, yaw, information);    // from a constant reference-frame node
//   int rc = graph.optimize(/*exclude_registration_constraints=*/false);
//   std::map<std::pair<int64_t, int64_t>, std::array<double, 16>> covariances = {{{first, second}, {}}};
//   bool usable = graph.getEdgeCovarianceMap(&covariances);             // pose_graph.cpp:117-163
//
// Error convention: nothing is thrown out of optimize(); it returns the library's status and last_error() its text.
#ifndef VOXGRAPH_AMD_CPP_GPU_POSE_GRAPH_H_
#define VOXGRAPH_AMD_CPP_GPU_POSE_GRAPH_H_

#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "voxgraph_amd.h"

namespace voxgraph_amd {

// Constraint::Constraint (constraint.cpp:4-38): sqrt_information = L^T of the LLT of the information matrix (row-major
// 4x4).  false when the matrix is not positive definite.
inline bool SqrtInformation(const double information[16], double sqrt_information[16]) {
  double L[16] = {0};
  for (int j = 0; j < 4; ++j) {
    double d = information[4 * j + j];
    for (int k = 0; k < j; ++k) d -= L[4 * j + k] * L[4 * j + k];
    if (!(d > 0.0) || std::isinf(d)) return false;
    L[4 * j + j] = std::sqrt(d);
    for (int i = j + 1; i < 4; ++i) {
      double v = information[4 * i + j];
      for (int k = 0; k < j; ++k) v -= L[4 * i + k] * L[4 * j + k];
      L[4 * i + j] = v / L[4 * j + j];
    }
  }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) sqrt_information[4 * i + j] = L[4 * j + i];
  return true;
}

// LoopClosureEdgeServer::publishLoopClosureEdges (loop_closure_edge_server.cpp:85-96): the 6x6 message covariance
// {x, y, z, roll, pitch, yaw} of a 4-DoF block {x, y, z, yaw} -- every entry `unknown`
// (kSetUnknownCovarianceEntriesTo), then the 4x4 into rows / columns {0, 1, 2, 5}.
inline void FillLoopClosureEdgeCovariance(const double cov4[16], double out36[36], double unknown = 1e4) {
  for (int i = 0; i < 36; ++i) out36[i] = unknown;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) out36[(r == 3 ? 5 : r) * 6 + (c == 3 ? 5 : c)] = cov4[4 * r + c];
}
// ... and :121-129, what it publishes when the covariances are not usable: the identity
inline void IdentityLoopClosureEdgeCovariance(double out36[36]) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) out36[r * 6 + c] = r == c ? 1.0 : 0.0;
}

class GpuPoseGraph {
 public:
  using EdgeCovarianceMap = std::map<std::pair<int64_t, int64_t>, std::array<double, 16>>;  // keys: submap ids
  using Pose = std::array<double, 4>;  // x, y, z, yaw
  explicit GpuPoseGraph(vgx_ctx ctx) : ctx_(ctx) { vgx_pose_graph_options_default(&options_); }
  GpuPoseGraph(const GpuPoseGraph&) = delete;
  GpuPoseGraph& operator=(const GpuPoseGraph&) = delete;
  ~GpuPoseGraph() { Release(); }

  vgx_pose_graph_options& options() { return options_; }
  // The linear solver of the next solves (include/voxgraph_amd.h, "Pose graph: the tile-sparse solver"):
  // VGX_LINEAR_SOLVER_DENSE (the default, 4096 free nodes at the most) or VGX_LINEAR_SOLVER_TILE_SPARSE with
  // VGX_ORDER_NATURAL or VGX_ORDER_RCM.  (VGX_ORDER_GIVEN is a permutation of the free nodes in the order they were
  // added: `permutation` is copied.)  getEdgeCovarianceMap follows the setting: the dense factor (and its limit) with
  // the dense solver, the tile-sparse factor (vgx_pose_graph_covariance_sparse, no free-node limit) with the other.
  // On a graph that stands (no node or constraint changed since the last solve) the setting goes to the live handle
  // (vgx_pose_graph_set_linear_solver: the registration batch is kept) and a refusal is returned at once, nothing
  // changed; otherwise it is kept for the next optimize(), which then reports a refusal.
  int setLinearSolver(int32_t solver, int32_t ordering = VGX_ORDER_NATURAL, const std::vector<int32_t>& permutation = {}) {
    if (graph_ && !dirty_) {
      size_t n_free = 0;
      for (int32_t c : constant_) n_free += c == 0;
      if (ordering == VGX_ORDER_GIVEN && permutation.size() != n_free) {
        Fail("setLinearSolver: the permutation's length is not the number of free nodes");
        return VGX_ERR_INVALID;
      }
      const int rc = vgx_pose_graph_set_linear_solver(graph_, solver, ordering, permutation.empty() ? nullptr : permutation.data());
      if (rc != VGX_OK) return Status(rc);
    }
    solver_ = solver;
    ordering_ = ordering;
    permutation_ = permutation;
    return VGX_OK;
  }
  // vgx_pose_graph_structure of the last solve; false before one, or with the dense solver
  bool getStructure(vgx_pose_graph_structure_stats* stats) {
    if (!graph_ || !stats) return Fail("getStructure: no solve yet or NULL stats");
    const int rc = vgx_pose_graph_structure(graph_, stats);
    if (rc != VGX_OK) Status(rc);
    return rc == VGX_OK;
  }

  // nodes: submaps and reference frames share one numbering, in the order they were added
  int addSubmapNode(int64_t submap_id, const Pose& pose, bool constant) { return AddNode(submap_index_, submap_id, pose, constant); }
  int addReferenceFrameNode(int64_t frame_id, const Pose& pose) { return AddNode(frame_index_, frame_id, pose, true); }
  bool hasSubmapNode(int64_t submap_id) const { return submap_index_.count(submap_id) != 0; }

  // registration constraints: cost functions the caller made and keeps (vgx_reg_create(ctx, reference, reading, ...)).
  // pose_graph.cpp:62-71 adds the MIRRORED constraint for isosurface points: pass the second cost function, built with
  // the submaps swapped, as `mirrored` (NULL otherwise).
  bool addRegistrationConstraint(vgx_reg reg, int64_t first_submap_id, int64_t second_submap_id, vgx_reg mirrored = nullptr) {
    if (!reg || !hasSubmapNode(first_submap_id) || !hasSubmapNode(second_submap_id)) return Fail("addRegistrationConstraint: unknown submap or NULL cost function");
    const int32_t a = submap_index_[first_submap_id], b = submap_index_[second_submap_id];
    regs_.push_back(reg);
    pairs_.push_back(a);
    pairs_.push_back(b);
    if (mirrored) {
      regs_.push_back(mirrored);
      pairs_.push_back(b);
      pairs_.push_back(a);
    }
    dirty_ = true;
    return true;
  }
  bool addRelativePoseConstraint(int64_t origin_submap_id, int64_t destination_submap_id, const double t[3], double yaw,
                                 const double information[16]) {
    if (!hasSubmapNode(origin_submap_id) || !hasSubmapNode(destination_submap_id)) return Fail("addRelativePoseConstraint: unknown submap");
    return AddEdge(submap_index_[origin_submap_id], submap_index_[destination_submap_id], t, yaw, information);
  }
  bool addAbsolutePoseConstraint(int64_t frame_id, int64_t submap_id, const double t[3], double yaw, const double information[16]) {
    if (!frame_index_.count(frame_id) || !hasSubmapNode(submap_id)) return Fail("addAbsolutePoseConstraint: unknown frame or submap");
    return AddEdge(frame_index_[frame_id], submap_index_[submap_id], t, yaw, information);
  }
  void resetRegistrationConstraints() {
    regs_.clear();
    pairs_.clear();
    dirty_ = true;
  }
  void resetRelativePoseConstraints() {
    edges_.clear();
    dirty_ = true;
  }

  // PoseGraph::optimize(bool exclude_registration_constraints): VGX_OK or the library's status; never throws
  int optimize(bool exclude_registration_constraints = false) {
    int rc = Build();
    if (rc != VGX_OK) return rc;
    vgx_pose_graph_options opt = options_;
    opt.exclude_registration_constraints = exclude_registration_constraints ? 1 : 0;
    vgx_pose_graph_summary summary;
    rc = vgx_pose_graph_optimize(graph_, &opt, poses_.data(), &summary);
    if (rc != VGX_OK) return Status(rc);
    summaries_.push_back(summary);
    return VGX_OK;
  }
  std::map<int64_t, Pose> getSubmapPoses() const {
    std::map<int64_t, Pose> out;
    for (const auto& kv : submap_index_) {
      Pose p;
      for (int k = 0; k < 4; ++k) p[k] = poses_[4 * static_cast<size_t>(kv.second) + k];
      out[kv.first] = p;
    }
    return out;
  }
  // PoseGraph::getEdgeCovarianceMap (pose_graph.cpp:117-163): for every key (first, second) of the map the row-major 4x4
  // covariance block of the two submap poses, from one evaluation of the whole problem (registration constraints
  // included) at the current poses.  false -- the map is then not to be used -- on an unknown submap id or a failed
  // computation (a rank-deficient graph; last_error() says which).  With the tile-sparse solver the columns are solved
  // on the sparse factor, in slabs of at most `max_solve_bytes` (0: the library's default); lastCovarianceStats() tells
  bool getEdgeCovarianceMap(EdgeCovarianceMap* map, int64_t max_solve_bytes = 0) {
    if (!map) return Fail("getEdgeCovarianceMap: NULL map");
    std::vector<int32_t> pairs;
    for (const auto& kv : *map) {
      if (!hasSubmapNode(kv.first.first) || !hasSubmapNode(kv.first.second)) return Fail("getEdgeCovarianceMap: unknown submap");
      pairs.push_back(submap_index_[kv.first.first]);
      pairs.push_back(submap_index_[kv.first.second]);
    }
    if (pairs.empty()) return true;
    if (Build() != VGX_OK) return false;
    std::vector<double> blocks(8 * pairs.size());
    const int32_t n_pairs = static_cast<int32_t>(pairs.size() / 2);
    covariance_stats_ = vgx_pose_graph_covariance_stats();
    const int rc = solver_ == VGX_LINEAR_SOLVER_TILE_SPARSE
                       ? vgx_pose_graph_covariance_sparse(graph_, poses_.data(), 0, n_pairs, pairs.data(), max_solve_bytes, blocks.data(),
                                                          &covariance_stats_)
                       : vgx_pose_graph_covariance(graph_, poses_.data(), 0, n_pairs, pairs.data(), blocks.data());
    if (rc != VGX_OK) {
      Status(rc);
      return false;
    }
    size_t p = 0;
    for (auto& kv : *map) {
      for (int k = 0; k < 16; ++k) kv.second[static_cast<size_t>(k)] = blocks[16 * p + static_cast<size_t>(k)];
      ++p;
    }
    return true;
  }
  // what the last getEdgeCovarianceMap on the tile-sparse factor solved (columns, slabs, launches, bytes); zeros after
  // one on the dense factor
  const vgx_pose_graph_covariance_stats& lastCovarianceStats() const { return covariance_stats_; }
  const std::vector<vgx_pose_graph_summary>& getSolverSummaries() const { return summaries_; }
  std::vector<vgx_pose_graph_iteration> lastHistory() const {
    int32_t n = 0;
    std::vector<vgx_pose_graph_iteration> out;
    if (!graph_ || vgx_pose_graph_history(graph_, 0, nullptr, &n) != VGX_OK || n == 0) return out;
    out.resize(static_cast<size_t>(n));
    vgx_pose_graph_history(graph_, n, out.data(), nullptr);
    return out;
  }
  const std::string& last_error() const { return error_; }

 private:
  int AddNode(std::map<int64_t, int32_t>& index, int64_t id, const Pose& pose, bool constant) {
    auto it = index.find(id);
    if (it != index.end()) {  // PoseGraph::addSubmapNode replaces a node that exists
      for (int k = 0; k < 4; ++k) poses_[4 * static_cast<size_t>(it->second) + k] = pose[k];
      dirty_ = dirty_ || (constant_[static_cast<size_t>(it->second)] != 0) != constant;
      constant_[static_cast<size_t>(it->second)] = constant ? 1 : 0;
      return it->second;
    }
    const int32_t node = static_cast<int32_t>(constant_.size());
    index[id] = node;
    constant_.push_back(constant ? 1 : 0);
    poses_.insert(poses_.end(), pose.begin(), pose.end());
    dirty_ = true;
    return node;
  }
  bool AddEdge(int32_t a, int32_t b, const double t[3], double yaw, const double information[16]) {
    vgx_pose_graph_edge e;
    e.a = a;
    e.b = b;
    for (int k = 0; k < 3; ++k) e.t_obs[k] = t[k];
    e.yaw_obs = yaw;
    if (!SqrtInformation(information, e.sqrt_information)) return Fail("the information matrix is not positive definite");
    edges_.push_back(e);
    dirty_ = true;
    return true;
  }
  // the handles follow the lists: rebuilt when nodes or constraints changed since the last solve
  // (vgx_pose_graph_set_edges refuses an edge whose t_obs, yaw_obs or sqrt_information is not finite: optimize() then
  // returns VGX_ERR_INVALID and last_error() says which edge)
  int Build() {
    if (!dirty_ && graph_) return VGX_OK;
    Release();
    size_t n_free = 0;
    for (int32_t c : constant_) n_free += c == 0;
    if (ordering_ == VGX_ORDER_GIVEN && permutation_.size() != n_free) {
      Fail("setLinearSolver: the permutation's length is not the number of free nodes");
      return VGX_ERR_INVALID;
    }
    int rc = vgx_pose_graph_create_with_solver(ctx_, static_cast<int32_t>(constant_.size()), constant_.data(), solver_, ordering_,
                                               permutation_.empty() ? nullptr : permutation_.data(), &graph_);
    if (rc != VGX_OK) return Status(rc);
    if (!regs_.empty()) {
      rc = vgx_reg_batch_create(ctx_, static_cast<int32_t>(regs_.size()), regs_.data(), pairs_.data(), nullptr,
                                static_cast<int32_t>(regs_.size()), &batch_);
      if (rc != VGX_OK) return Status(rc);
      rc = vgx_pose_graph_set_registration(graph_, batch_);
      if (rc != VGX_OK) return Status(rc);
    }
    rc = vgx_pose_graph_set_edges(graph_, static_cast<int32_t>(edges_.size()), edges_.data());
    if (rc != VGX_OK) return Status(rc);
    dirty_ = false;
    return VGX_OK;
  }
  void Release() {
    if (graph_) vgx_pose_graph_destroy(graph_);
    if (batch_) vgx_reg_batch_destroy(batch_);
    graph_ = nullptr;
    batch_ = nullptr;
  }
  int Status(int rc) {
    error_ = vgx_last_error(ctx_);
    return rc;
  }
  bool Fail(const char* what) {
    error_ = what;
    return false;
  }

  vgx_ctx ctx_;
  vgx_pose_graph graph_ = nullptr;
  vgx_reg_batch batch_ = nullptr;
  vgx_pose_graph_options options_;
  int32_t solver_ = VGX_LINEAR_SOLVER_DENSE, ordering_ = VGX_ORDER_NATURAL;
  std::vector<int32_t> permutation_;
  std::map<int64_t, int32_t> submap_index_, frame_index_;
  std::vector<int32_t> constant_;
  std::vector<double> poses_;
  std::vector<vgx_reg> regs_;
  std::vector<int32_t> pairs_;
  std::vector<vgx_pose_graph_edge> edges_;
  std::vector<vgx_pose_graph_summary> summaries_;
  vgx_pose_graph_covariance_stats covariance_stats_ = vgx_pose_graph_covariance_stats();
  bool dirty_ = true;
  std::string error_;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_POSE_GRAPH_H_
