// GpuViewRenderer (voxgraph_amd/cpp/gpu_view_renderer.h) from plain C++, for tests/test_view_render_cpp.py.
//   view_render_smoke compile     no device: every overload instantiates; the config's defaults; the ray helpers
//   view_render_smoke IN OUT      integrates the scans of IN into one layer (reproducible mode), renders the view, hands
//                                 its points to a registerer and to a second layer's integrator, and writes OUT
// IN: int32 n_scans, vps, image_width; f32 voxel_size, max_abs_distance, min_range; f32 s_min, s_max, step_scale, min_step,
//     unknown_step, max_bracket; per scan: f32 T[7], int64 n, f32 points [n][3]; f32 T_view[7]; int64 n_dirs,
//     f32 dirs [n_dirs][3]; f32 prior[7]
// OUT: int64 counts[8]; f32 range [n]; u8 status [n]; f32 points [n][3]; f32 gradient [n][3]; f32 weight [n]; u32 rgba [n];
//      int32 n_samples [n]; int32 usable; f32 T_refined[7]; int32 blocks of the second layer
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_view_renderer.h"

namespace {
using voxgraph_amd::GpuViewRenderer;

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}

// kindr's transformation, as far as the renderer reads it
struct Quat {
  float w_, x_, y_, z_;
  float w() const { return w_; }
  float x() const { return x_; }
  float y() const { return y_; }
  float z() const { return z_; }
};
struct Position {
  float v[3];
  float operator[](int k) const { return v[k]; }
};
struct Transformation {
  Quat q;
  Position p;
  const Quat& getRotation() const { return q; }
  const Position& getPosition() const { return p; }
};

// never called without a device: the overloads only have to instantiate
bool instantiate(GpuViewRenderer* r, const voxgraph_amd::GpuTsdfLayer& layer, vgx_submap submap,
                 voxgraph_amd::GpuScanToMapRegisterer* registerer, voxgraph_amd::GpuFastTsdfIntegrator* integrator) {
  float T[7] = {1, 0, 0, 0, 0, 0, 0};
  const Transformation A{{1, 0, 0, 0}, {{0, 0, 0}}};
  int64_t rays = r->render(layer, T).n_rays;
  rays += r->render(submap, T).n_rays;
  rays += r->render(layer, A).n_rays;
  rays += r->render(submap, A).n_rays;
  const bool usable = r->renderInto(registerer, T, T);
  r->renderInto(integrator, T);
  r->download(nullptr, nullptr);
  return usable && rays > 0 && r->devicePoints() != nullptr && r->lastCounts().n_hit > 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "compile") == 0) {
    const GpuViewRenderer::Config c = GpuViewRenderer::defaultConfig(12.0f, 0.05f, 0.2f, 0.6f);
    GpuViewRenderer::Config none;
    vgx_view_config_default(&none);
    vgx_view view = nullptr;
    const int refused = vgx_view_create(nullptr, &c, &view);  // (no context: refused before anything else)
    const std::vector<float> pin = GpuViewRenderer::pinholeRays(4, 3, 2.0, 2.0, 1.5, 1.0), lid = GpuViewRenderer::lidarRays(8, 2, -0.1, 0.1);
    bool unit = pin.size() == 36 && lid.size() == 48;
    for (size_t i = 0; i + 2 < pin.size(); i += 3)
      unit = unit && std::fabs(std::sqrt((double)pin[i] * pin[i] + (double)pin[i + 1] * pin[i + 1] + (double)pin[i + 2] * pin[i + 2]) - 1.0) < 1e-6;
    bool (*keep)(GpuViewRenderer*, const voxgraph_amd::GpuTsdfLayer&, vgx_submap, voxgraph_amd::GpuScanToMapRegisterer*,
                 voxgraph_amd::GpuFastTsdfIntegrator*) = &instantiate;
    printf("VIEW_RENDER_COMPILE_OK %d %d %d %d %d %d\n", c.s_min == 0.0f && c.step_scale == 0.75f, c.image_width == 0 && c.flags == VGX_VIEW_POINTS,
           none.s_max == 0.0f && none.min_step == 0.0f && none.unknown_step == 0.0f && none.max_bracket == 0.0f,
           vgx_view_config_check(&c) == VGX_OK && vgx_view_config_check(&none) == VGX_ERR_INVALID, unit,
           refused == VGX_ERR_INVALID && view == nullptr && keep != nullptr);
    return 0;
  }
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t n_scans = 0, vps = 0, image_width = 0;
  float vs = 0, max_abs = 0, min_range = 0, s[6];
  if (!rd(in, &n_scans, 1) || !rd(in, &vps, 1) || !rd(in, &image_width, 1) || !rd(in, &vs, 1) || !rd(in, &max_abs, 1) ||
      !rd(in, &min_range, 1) || !rd(in, s, 6))
    return 3;
  std::vector<std::vector<float>> poses((size_t)n_scans, std::vector<float>(7)), scans((size_t)n_scans);
  for (int k = 0; k < n_scans; ++k) {
    int64_t n = 0;
    if (!rd(in, poses[k].data(), 7) || !rd(in, &n, 1)) return 3;
    scans[k].resize(3 * (size_t)n);
    if (!rd(in, scans[k].data(), scans[k].size())) return 3;
  }
  float T_view[7], prior[7];
  int64_t n = 0;
  if (!rd(in, T_view, 7) || !rd(in, &n, 1)) return 3;
  std::vector<float> dirs(3 * (size_t)n);
  if (!rd(in, dirs.data(), dirs.size()) || !rd(in, prior, 7)) return 3;
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 7;
  try {
    voxgraph_amd::GpuTsdfLayer layer(ctx, vs, vps), second(ctx, vs, vps);
    voxgraph_amd::GpuFastTsdfIntegrator::Config cfg = voxgraph_amd::GpuFastTsdfIntegrator::defaultConfig();
    cfg.default_truncation_distance = 0.6f;  // voxgraph_mapper.yaml:21-28
    cfg.max_ray_length_m = 16.0f;
    cfg.use_const_weight = 1;
    cfg.use_weight_dropoff = 1;
    cfg.use_sparsity_compensation_factor = 1;
    cfg.sparsity_compensation_factor = 20.0f;
    cfg.deterministic = 1;
    voxgraph_amd::GpuFastTsdfIntegrator integrator(ctx, cfg, &layer), into(ctx, cfg, &second);
    for (int k = 0; k < n_scans; ++k)
      integrator.integratePointCloud(poses[k].data(), scans[k].data(), nullptr, (int64_t)(scans[k].size() / 3));
    GpuViewRenderer::Config vc = GpuViewRenderer::defaultConfig(s[1], s[3], s[4], s[5]);
    vc.s_min = s[0];
    vc.step_scale = s[2];
    vc.image_width = image_width;
    vc.flags = VGX_VIEW_ALL;
    GpuViewRenderer renderer(ctx, vc);
    renderer.setRays(dirs.data(), n);
    // the pose through the kindr-style overload
    const Transformation pose{{T_view[0], T_view[1], T_view[2], T_view[3]}, {{T_view[4], T_view[5], T_view[6]}}};
    const vgx_view_counts counts = renderer.render(layer, pose);
    if (counts.n_rays != n) return 6;
    const size_t un = (size_t)n;
    std::vector<float> range(un), points(3 * un), gradient(3 * un), weight(un);
    std::vector<uint8_t> status(un);
    std::vector<uint32_t> rgba(un);
    std::vector<int32_t> n_samples(un);
    renderer.download(range.data(), status.data(), points.data(), gradient.data(), weight.data(), rgba.data(), n_samples.data());
    fwrite(&counts, sizeof(counts), 1, out);
    fwrite(range.data(), 4, un, out);
    fwrite(status.data(), 1, un, out);
    fwrite(points.data(), 4, 3 * un, out);
    fwrite(gradient.data(), 4, 3 * un, out);
    fwrite(weight.data(), 4, un, out);
    fwrite(rgba.data(), 4, un, out);
    fwrite(n_samples.data(), 4, un, out);
    voxgraph_amd::GpuScanToMapRegisterer::Config rc = voxgraph_amd::GpuScanToMapRegisterer::defaultConfig(max_abs);
    rc.min_range_m = min_range;
    voxgraph_amd::GpuScanToMapRegisterer registerer(ctx, rc, &layer);
    float refined[7];
    const int32_t usable = renderer.renderInto(&registerer, prior, refined) ? 1 : 0;
    fwrite(&usable, 4, 1, out);
    fwrite(refined, 4, 7, out);
    renderer.renderInto(&into, T_view);
    int32_t blocks = 0;
    int64_t dropped = 0;
    if (vgx_tsdf_layer_stats(second.handle(), &blocks, &dropped) != VGX_OK) return 8;
    fwrite(&blocks, 4, 1, out);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  fclose(out);
  vgx_ctx_destroy(ctx);
  printf("VIEW_RENDER_SMOKE_OK\n");
  return 0;
}
