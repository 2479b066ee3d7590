// What scan-to-map registration (vgx_scan_reg.hip: the active TSDF layer) and scan localisation
// (vgx_scan_localize.hip: posed finished submaps) share: the handle, the partition's constants, the points
// of an evaluation, and the trust-region loop on the host.  Both routes feed the loop one evaluation
// {15 sums, usable points, candidates}; everything after that is the same code.
#ifndef VGX_SCAN_REG_INTERNAL_H_
#define VGX_SCAN_REG_INTERNAL_H_

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "vgx_internal.h"
#include "vgx_pose.h"

namespace vgx {

constexpr int kScanRegThreads = 256;
constexpr int kScanRegTrips = 4;                                  // candidates per thread
constexpr int kScanRegQuota = kScanRegThreads * kScanRegTrips;    // candidates per workgroup
constexpr int kScanRegFold = 256;                                 // threads of the fold: its width
constexpr int kScanRegSums = 15;

struct ScanRegPartial {  // 136 B
  double s[kScanRegSums];
  long long n_valid, n_candidates;
};

constexpr int kScanMapMaxSubmaps = 64;

// one posed finished submap as the localisation kernels read it: its block table, the chosen raw layer, T_S_M
// (mission-frame points into the submap frame) and the rotation of T_M_S (gradients back)
struct ScanMapSubmapDev : LayerTable {
  const float* val;  // ESDF or TSDF distance
  const void* vld;   // ESDF observed (uint8) or TSDF weight (float)
  float q_sm[4], t_sm[3];
  float q_ms[4];
};

}  // namespace vgx

struct vgx_scan_registration_s {
  vgx_ctx ctx = nullptr;
  vgx_scan_registration_config cfg{};
  std::mutex mu;  // one call at a time per handle
  enum Source { kNone, kOwned, kDevice, kScan } source = kNone;
  vgx::DeviceBuffer d_points;         // kOwned: the host points' copy
  const void* borrowed = nullptr;  // kDevice
  vgx_scan scan = nullptr;       // kScan
  int64_t n = 0;                 // kOwned / kDevice
  vgx::DeviceBuffer d_partials;       // ScanRegPartial [workgroups], grown on demand
  vgx::DeviceBuffer d_out;            // ScanRegPartial: the totals
  vgx::PinnedBuffer h_out;            // ... and their pinned stage
  std::vector<vgx_pose_graph_iteration> history;
  // scan localisation (vgx_scan_localize.hip): the map set by vgx_scan_registration_set_map.  Each listed submap carries
  // one user count of this handle until the next set_map or the handle's destruction.
  vgx_scan_map_config map_cfg{};
  std::vector<vgx_submap> map_submaps;
  std::vector<vgx::ScanMapSubmapDev> map_desc;  // host copy: the layer pointers are filled in at every evaluation
  int32_t map_vps = 0;
  vgx::DeviceBuffer d_map_desc;       // ScanMapSubmapDev [n_submaps]
  vgx::DeviceBuffer d_map_partials;   // the map kernels' partials, grown on demand
  vgx::DeviceBuffer d_map_out;        // their totals: one per pose
  vgx::DeviceBuffer d_map_poses;      // float [n_poses][7]
  vgx::PinnedBuffer h_map_stage;      // the pose table on its way up, then the totals on their way down
};

namespace vgx {

inline int reg_fail(vgx_ctx ctx, const char* fn, const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": " + msg); }

inline double reg_seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

inline double reg_normalize_angle(double a) {
  const double two_pi = 2.0 * M_PI;
  return a - two_pi * std::floor((a + M_PI) / two_pi);
}

// a pose {qw,qx,qy,qz, tx,ty,tz}: finite, and the quaternion unit by the 1e-4 rule; else what is wrong with it
inline const char* reg_pose_error(const float* T) {
  const PoseDefect bad = pose_defect(T);
  return bad == kPoseNotFinite ? "is not finite" : bad == kPoseNotUnit ? "has a quaternion that is not unit (| |q|^2 - 1 | > 1e-4)" : nullptr;
}

// The points of this evaluation (R->mu held, no context lock held: a scan's own lock comes before them and is handed to
// the caller, who keeps it until the evaluation has run).  vgx_scan_reg.hip.
int reg_points(const char* fn, vgx_scan_registration R, const float** d_points, int64_t* n, std::unique_lock<std::mutex>* scan_lock);

// the listed submaps' user counts given back; carries out the vgx_submap_destroy calls deferred meanwhile.  vgx_scan_localize.hip.
void scan_map_release(vgx_scan_registration R);

// out[15] -> g [4], H [4][4] (both triangles)
inline void unpack_system(const double* s, double g[4], double H[4][4]) {
  for (int k = 0; k < 4; ++k) g[k] = s[1 + k];
  int e = 5;
  for (int k = 0; k < 4; ++k)
    for (int l = k; l < 4; ++l) {
      H[k][l] = s[e];
      H[l][k] = s[e++];
    }
}

// step = -A^-1 g, A = H + diag(clip(H_ii, 1e-6, 1e32) / radius): the unblocked right-looking Cholesky and the
// column-oriented substitutions of the pose-graph solve's order contract; false on a pivot that is not positive or not finite
inline bool damped_step(const double H[4][4], const double g[4], double radius, double step[4]) {
  double A[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) A[i][j] = H[i][j];
  for (int i = 0; i < 4; ++i) {
    const double d2 = std::min(std::max(H[i][i], 1e-6), 1e32);
    A[i][i] = H[i][i] + d2 / radius;
  }
  for (int k = 0; k < 4; ++k) {
    const double akk = A[k][k];
    if (!(akk > 0.0) || std::isinf(akk)) return false;
    A[k][k] = std::sqrt(akk);
    for (int i = k + 1; i < 4; ++i) A[i][k] = A[i][k] / A[k][k];
    for (int i = k + 1; i < 4; ++i)
      for (int j = k + 1; j <= i; ++j) A[i][j] = A[i][j] - A[i][k] * A[j][k];
  }
  double y[4] = {g[0], g[1], g[2], g[3]};
  for (int j = 0; j < 4; ++j) {
    y[j] = y[j] / A[j][j];
    for (int i = j + 1; i < 4; ++i) y[i] = y[i] - A[i][j] * y[j];
  }
  for (int j = 3; j >= 0; --j) {
    y[j] = y[j] / A[j][j];
    for (int i = 0; i < j; ++i) y[i] = y[i] - A[j][i] * y[j];
  }
  for (int i = 0; i < 4; ++i) step[i] = -y[i];
  return true;
}

// The loop and the outcome rule ("Scan-to-map registration", THE LOOP / THE OUTCOME) over any evaluation
// `int evaluate(const double x[4], ScanRegPartial* tot)`: n_valid the usable points, n_candidates the candidates.  Writes
// T_refined, delta_out, the handle's history and (nullable) the summary.
template <class Evaluate>
int reg_refine_loop(vgx_scan_registration R, const float T[7], const vgx_pose_graph_options& opt, Evaluate&& evaluate_at,
                    float T_refined[7], double delta_out[4], vgx_scan_registration_summary* summary) {
  const auto t0 = std::chrono::steady_clock::now();
  vgx_scan_registration_summary S;
  std::memset(&S, 0, sizeof(S));
  std::vector<vgx_pose_graph_iteration> history;
  double eval_seconds = 0.0;
  auto evaluate = [&](const double x[4], ScanRegPartial* tot) {
    const auto e0 = std::chrono::steady_clock::now();
    const int r = evaluate_at(x, tot);
    eval_seconds += reg_seconds_since(e0);
    ++S.num_evaluations;
    return r;
  };
  auto enough = [&](const ScanRegPartial& p) {
    return p.n_candidates > 0 && (double)p.n_valid / (double)p.n_candidates >= (double)R->cfg.min_valid_ratio;
  };
  double x[4] = {0.0, 0.0, 0.0, 0.0}, cand[4], g[4], H[4][4];
  ScanRegPartial cur;
  int rc = evaluate(x, &cur);
  if (rc != VGX_OK) return rc;
  double cost = 0.5 * cur.s[0];
  S.n_candidates = cur.n_candidates;
  S.n_valid_first = S.n_valid_last = cur.n_valid;
  S.initial_cost = cost;
  int it = 0, reason = VGX_TERMINATION_MAX_ITERATIONS;
  const bool enough_first = enough(cur);
  if (!enough_first) {
    reason = VGX_TERMINATION_TOO_FEW_POINTS;
  } else {
    unpack_system(cur.s, g, H);
    double radius = opt.initial_trust_region_radius, decrease = 2.0;
    while (it < opt.max_num_iterations) {
      ++it;
      history.push_back(vgx_pose_graph_iteration{cost, 0.0, 0.0, radius, 0.0, 0, 0});
      vgx_pose_graph_iteration& rec = history.back();
      double gmax = 0.0;  // a NaN stays: it is not <= the tolerance
      for (int i = 0; i < 4; ++i) {
        const double a = std::fabs(g[i]);
        if (a > gmax || std::isnan(a)) gmax = a;
      }
      if (gmax <= opt.gradient_tolerance) {
        reason = VGX_TERMINATION_GRADIENT_TOLERANCE;
        break;
      }
      double step[4];
      if (!damped_step(H, g, radius, step)) {
        rec.factorization_failed = 1;
        ++S.num_factorization_failures;
        radius /= decrease;
        decrease *= 2.0;
        continue;
      }
      double Hs[4];
      for (int i = 0; i < 4; ++i) {  // per row, ascending columns, from 0.0
        double a = 0.0;
        for (int c = 0; c < 4; ++c) a = a + H[i][c] * step[c];
        Hs[i] = a;
      }
      double s2 = 0.0, x2 = 0.0;
      for (int i = 0; i < 4; ++i) s2 = s2 + step[i] * step[i];
      for (int i = 0; i < 4; ++i) x2 = x2 + x[i] * x[i];
      const double step_norm = std::sqrt(s2);
      rec.step_norm = step_norm;
      if (step_norm <= opt.parameter_tolerance * (std::sqrt(x2) + opt.parameter_tolerance)) {
        reason = VGX_TERMINATION_PARAMETER_TOLERANCE;
        break;
      }
      for (int i = 0; i < 4; ++i) cand[i] = x[i] + step[i];
      cand[3] = reg_normalize_angle(cand[3]);
      ScanRegPartial tri;
      rc = evaluate(cand, &tri);
      if (rc != VGX_OK) return rc;
      const double trial = 0.5 * tri.s[0];
      double gs = 0.0, sHs = 0.0;
      for (int i = 0; i < 4; ++i) gs = gs + g[i] * step[i];
      for (int i = 0; i < 4; ++i) sHs = sHs + step[i] * Hs[i];
      const double model_decrease = -(gs + 0.5 * sHs);
      const double rho = model_decrease > 0.0 ? (cost - trial) / model_decrease : -1.0;
      rec.trial_cost = trial;
      rec.gain_ratio = rho;
      if (rho > 1e-3) {
        rec.accepted = 1;
        ++S.num_successful_steps;
        const double rel = std::fabs(cost - trial) / std::max(cost, 1e-300);
        for (int i = 0; i < 4; ++i) x[i] = cand[i];
        cost = trial;
        cur = tri;
        unpack_system(cur.s, g, H);
        const double q = 2.0 * rho - 1.0;
        radius = std::min(radius / std::max(1.0 / 3.0, 1.0 - q * q * q), 1e16);
        decrease = 2.0;
        if (rel <= opt.function_tolerance) {
          reason = VGX_TERMINATION_FUNCTION_TOLERANCE;
          break;
        }
      } else {
        radius /= decrease;
        decrease *= 2.0;
      }
      if (reg_seconds_since(t0) > opt.max_solver_time_in_seconds) {
        reason = VGX_TERMINATION_MAX_SOLVER_TIME;
        break;
      }
    }
  }
  S.termination_reason = reason;
  S.termination_type = reason == VGX_TERMINATION_TOO_FEW_POINTS ? VGX_FAILURE
                       : reason <= VGX_TERMINATION_GRADIENT_TOLERANCE ? VGX_CONVERGENCE
                                                                      : VGX_NO_CONVERGENCE;
  S.num_iterations = it;
  S.n_valid_last = cur.n_valid;
  S.final_cost = cost;
  S.usable = S.termination_type == VGX_CONVERGENCE && enough_first && enough(cur) ? 1 : 0;
  for (int k = 0; k < 7; ++k) T_refined[k] = T[k];
  if (S.usable) {
    // q_z(yaw) (x) q_prior and t_prior + delta in f64 from the f32 prior, rounded once
    const double cz = std::cos(0.5 * x[3]), sz = std::sin(0.5 * x[3]);
    const double w = T[0], qx = T[1], qy = T[2], qz = T[3];
    T_refined[0] = (float)(cz * w - sz * qz);
    T_refined[1] = (float)(cz * qx - sz * qy);
    T_refined[2] = (float)(cz * qy + sz * qx);
    T_refined[3] = (float)(cz * qz + sz * w);
    for (int a = 0; a < 3; ++a) T_refined[4 + a] = (float)((double)T[4 + a] + x[a]);
  }
  for (int k = 0; k < 4; ++k) delta_out[k] = x[k];
  S.evaluation_seconds = eval_seconds;
  S.total_seconds = reg_seconds_since(t0);
  R->history.swap(history);
  if (summary) *summary = S;
  return VGX_OK;
}

}  // namespace vgx

#endif  // VGX_SCAN_REG_INTERNAL_H_
