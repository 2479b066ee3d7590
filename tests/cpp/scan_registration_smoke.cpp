// GpuScanToMapRegisterer (voxgraph_amd/cpp/gpu_scan_to_map_registerer.h) from plain C++, for
// tests/test_scan_registration_cpp.py.
//   scan_registration_smoke compile     no device: every overload instantiates; the config's defaults
//   scan_registration_smoke IN OUT      integrates the scans of IN into one layer (reproducible mode), then refines every
//                                       prior against it and writes the results to OUT
// IN: int32 n_scans, vps, n_priors; f32 voxel_size, max_abs_distance; per scan: f32 T[7], int64 n, f32 points [n][3];
//     the scan to register: int64 n, f32 points [n][3]; f32 priors [n_priors][7]
// OUT: per prior: int32 usable, f32 T_refined[7], f64 delta[4]   (the last prior through the kindr-style overload)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_scan_to_map_registerer.h"

namespace {
using voxgraph_amd::GpuScanToMapRegisterer;

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}

// kindr's transformation, as far as the mirror reads and makes it
struct Quat {
  float w_, x_, y_, z_;
  Quat(float w, float x, float y, float z) : w_(w), x_(x), y_(y), z_(z) {}
  float w() const { return w_; }
  float x() const { return x_; }
  float y() const { return y_; }
  float z() const { return z_; }
};
struct Position {
  float v[3];
  Position(float x, float y, float z) : v{x, y, z} {}
  float operator[](int k) const { return v[k]; }
};
struct Transformation {
  Quat q;
  Position p;
  Transformation(const Quat& q_, const Position& p_) : q(q_), p(p_) {}
  const Quat& getRotation() const { return q; }
  const Position& getPosition() const { return p; }
};
struct Point {
  float x, y, z;
};

// never called without a device: the overloads only have to instantiate
bool instantiate(GpuScanToMapRegisterer* r, vgx_scan scan, const std::vector<Point>& cloud) {
  float T[7] = {1, 0, 0, 0, 0, 0, 0};
  Transformation A(Quat(1, 0, 0, 0), Position(0, 0, 0)), B = A;
  bool ok = r->refineSensorPose(scan, T, T);
  ok = r->refineSensorPose(&cloud[0].x, (int64_t)cloud.size(), T, T) && ok;
  ok = r->refineSensorPose(cloud, T, T) && ok;
  ok = r->refineSensorPose(cloud, A, &B) && ok;
  ok = r->refineSensorPose(scan, A, &B) && ok;
  return ok;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "compile") == 0) {
    const GpuScanToMapRegisterer::Config c = GpuScanToMapRegisterer::defaultConfig(0.55f);
    vgx_scan_registration reg = nullptr;
    GpuScanToMapRegisterer::Config none;
    vgx_scan_registration_config_default(&none);
    const int refused = vgx_scan_registration_create(nullptr, &none, &reg);  // (no context: refused before anything else)
    bool (*keep)(GpuScanToMapRegisterer*, vgx_scan, const std::vector<Point>&) = &instantiate;
    printf("SCAN_REGISTRATION_COMPILE_OK %d %d %d %d %d %d\n", c.min_range_m == 0.0f, std::isinf(c.max_range_m) && c.max_range_m > 0,
           c.point_stride, c.min_valid_ratio == 0.5f, none.max_abs_distance_m == 0.0f, refused == VGX_ERR_INVALID && keep != nullptr);
    return 0;
  }
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t n_scans = 0, vps = 0, n_priors = 0;
  float vs = 0, max_abs = 0;
  if (!rd(in, &n_scans, 1) || !rd(in, &vps, 1) || !rd(in, &n_priors, 1) || !rd(in, &vs, 1) || !rd(in, &max_abs, 1)) return 3;
  std::vector<std::vector<float>> poses((size_t)n_scans, std::vector<float>(7)), scans((size_t)n_scans);
  for (int k = 0; k < n_scans; ++k) {
    int64_t n = 0;
    if (!rd(in, poses[k].data(), 7) || !rd(in, &n, 1)) return 3;
    scans[k].resize(3 * (size_t)n);
    if (!rd(in, scans[k].data(), scans[k].size())) return 3;
  }
  int64_t n = 0;
  if (!rd(in, &n, 1)) return 3;
  std::vector<Point> cloud((size_t)n);
  if (!rd(in, cloud.data(), cloud.size())) return 3;
  std::vector<float> priors(7 * (size_t)n_priors);
  if (!rd(in, priors.data(), priors.size())) return 3;
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 7;
  try {
    voxgraph_amd::GpuTsdfLayer layer(ctx, vs, vps);
    voxgraph_amd::GpuFastTsdfIntegrator::Config cfg = voxgraph_amd::GpuFastTsdfIntegrator::defaultConfig();
    cfg.default_truncation_distance = 0.6f;  // voxgraph_mapper.yaml:21-28
    cfg.max_ray_length_m = 16.0f;
    cfg.use_const_weight = 1;
    cfg.use_weight_dropoff = 1;
    cfg.use_sparsity_compensation_factor = 1;
    cfg.sparsity_compensation_factor = 20.0f;
    cfg.deterministic = 1;
    voxgraph_amd::GpuFastTsdfIntegrator integrator(ctx, cfg, &layer);
    for (int k = 0; k < n_scans; ++k)
      integrator.integratePointCloud(poses[k].data(), scans[k].data(), nullptr, (int64_t)(scans[k].size() / 3));
    GpuScanToMapRegisterer registerer(ctx, GpuScanToMapRegisterer::defaultConfig(max_abs), &layer);
    for (int k = 0; k < n_priors; ++k) {
      const float* P = &priors[7 * (size_t)k];
      float T[7];
      int32_t usable = 0;
      if (k + 1 < n_priors) {
        usable = registerer.refineSensorPose(cloud, P, T) ? 1 : 0;
      } else {
        const Transformation prior(Quat(P[0], P[1], P[2], P[3]), Position(P[4], P[5], P[6]));
        Transformation refined = prior;
        usable = registerer.refineSensorPose(cloud, prior, &refined) ? 1 : 0;
        const float R[7] = {refined.q.w(), refined.q.x(), refined.q.y(), refined.q.z(), refined.p[0], refined.p[1], refined.p[2]};
        std::memcpy(T, R, sizeof(T));
      }
      fwrite(&usable, 4, 1, out);
      fwrite(T, 4, 7, out);
      fwrite(registerer.lastCorrection(), 8, 4, out);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  fclose(out);
  vgx_ctx_destroy(ctx);
  printf("SCAN_REGISTRATION_SMOKE_OK\n");
  return 0;
}
