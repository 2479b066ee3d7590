// GpuScanLocalizer (voxgraph_amd/cpp/gpu_scan_localizer.h) from plain C++, for tests/test_scan_localization_cpp.py.
//   scan_localization_smoke compile     no device: the defaults, the hypothesis grid, a NULL handle refused
//   scan_localization_smoke IN OUT      uploads the submap of IN, scores the grid of IN against it, refines the best
//                                       hypothesis and writes the grid and the results to OUT
// IN: int32 vps, n_blocks, score_point_stride, n_yaw; f32 voxel_size, max_abs_distance; f64 x_min, x_max, y_min, y_max, step, z;
//     int32 block_index [n][3]; f32 tsdf_distance, tsdf_weight, esdf_distance [n][vps^3]; u8 esdf_observed [n][vps^3];
//     int64 n_points; f32 points [n_points][3]
// OUT: int32 n_poses; f32 poses [n_poses][7]; int32 best_index, usable; f32 T_refined[7]; f64 delta[4];
//      f64 cost [n_poses]; int64 n_terms [n_poses]
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_scan_localizer.h"

namespace {
using voxgraph_amd::GpuScanLocalizer;
using voxgraph_amd::HypothesisGrid;

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "compile") == 0) {
    const GpuScanLocalizer::Config c = GpuScanLocalizer::defaultConfig(1.9f);
    const GpuScanLocalizer::MapConfig m = GpuScanLocalizer::defaultMapConfig();
    HypothesisGrid g;
    g.x_min = -1.0;
    g.x_max = 0.0;
    g.y_min = 2.0;
    g.y_max = 2.0;
    g.step = 0.5;
    g.n_yaw = 4;
    g.z = 0.25;
    const std::vector<float> poses = voxgraph_amd::makeHypothesisGrid(g);
    // 3 x 1 x 4 poses; the last one: x = 0, y = 2, yaw = 3 pi / 2
    const bool grid_ok = poses.size() == 7 * 12 && poses[7 * 11 + 4] == 0.0f && poses[7 * 11 + 5] == 2.0f && poses[7 * 11 + 6] == 0.25f &&
                         std::fabs(poses[7 * 11] - std::cos(0.75 * M_PI)) < 1e-6 && std::fabs(poses[7 * 11 + 3] - std::sin(0.75 * M_PI)) < 1e-6 &&
                         poses[0] == 1.0f && poses[4] == -1.0f;
    const float T[7] = {1, 0, 0, 0, 0, 0, 0};
    const int refused = vgx_scan_registration_set_map(nullptr, &m, 0, nullptr, nullptr);  // (no handle: refused before anything else)
    int32_t best = 0;
    float Tr[7];
    double delta[4];
    const int refused2 = vgx_scan_registration_localize(nullptr, 1, T, nullptr, &best, Tr, delta, nullptr);
    printf("SCAN_LOCALIZATION_COMPILE_OK %d %d %d %d %d %d\n", m.layer == VGX_EVAL_LAYER_ESDF, std::isinf(m.huber_delta_m) && m.huber_delta_m > 0,
           m.score_point_stride, c.max_abs_distance_m == 1.9f && c.min_valid_ratio == 0.5f, grid_ok,
           refused == VGX_ERR_INVALID && refused2 == VGX_ERR_INVALID);
    return 0;
  }
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t vps = 0, n_blocks = 0, stride = 0, n_yaw = 0;
  float vs = 0, max_abs = 0;
  double box[6];
  if (!rd(in, &vps, 1) || !rd(in, &n_blocks, 1) || !rd(in, &stride, 1) || !rd(in, &n_yaw, 1) || !rd(in, &vs, 1) || !rd(in, &max_abs, 1) ||
      !rd(in, box, 6))
    return 3;
  const size_t nvox = (size_t)n_blocks * vps * vps * vps;
  std::vector<int32_t> block_index(3 * (size_t)n_blocks);
  std::vector<float> td(nvox), tw(nvox), ed(nvox);
  std::vector<uint8_t> eo(nvox);
  int64_t n = 0;
  if (!rd(in, block_index.data(), block_index.size()) || !rd(in, td.data(), nvox) || !rd(in, tw.data(), nvox) || !rd(in, ed.data(), nvox) ||
      !rd(in, eo.data(), nvox) || !rd(in, &n, 1))
    return 3;
  std::vector<float> points(3 * (size_t)n);
  if (!rd(in, points.data(), points.size())) return 3;
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  vgx_submap sm = nullptr;
  if (vgx_submap_create(ctx, 0, vs, vps, n_blocks, block_index.data(), td.data(), tw.data(), ed.data(), eo.data(), &sm) != VGX_OK) return 4;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 7;
  try {
    GpuScanLocalizer localizer(ctx, GpuScanLocalizer::defaultConfig(max_abs));
    GpuScanLocalizer::MapConfig mc = GpuScanLocalizer::defaultMapConfig();
    mc.score_point_stride = stride;
    localizer.setMap(mc, {sm}, {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f});
    localizer.setPoints(points.data(), n);
    HypothesisGrid g;
    g.x_min = box[0];
    g.x_max = box[1];
    g.y_min = box[2];
    g.y_max = box[3];
    g.step = box[4];
    g.z = box[5];
    g.n_yaw = n_yaw;
    const std::vector<float> poses = voxgraph_amd::makeHypothesisGrid(g);
    const voxgraph_amd::ScanPoseScores scores = localizer.scorePoses(poses);
    const voxgraph_amd::ScanLocalizerResult r = localizer.localize(poses);
    const int32_t n_poses = (int32_t)(poses.size() / 7), usable = r.usable ? 1 : 0;
    fwrite(&n_poses, 4, 1, out);
    fwrite(poses.data(), 4, poses.size(), out);
    fwrite(&r.best_index, 4, 1, out);
    fwrite(&usable, 4, 1, out);
    fwrite(r.T_M_C, 4, 7, out);
    fwrite(r.delta, 8, 4, out);
    fwrite(scores.cost.data(), 8, scores.cost.size(), out);
    fwrite(scores.n_terms.data(), 8, scores.n_terms.size(), out);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  fclose(out);
  vgx_submap_destroy(sm);
  vgx_ctx_destroy(ctx);
  printf("SCAN_LOCALIZATION_SMOKE_OK\n");
  return 0;
}
