// voxgraph_amd::GpuPointcloudIntegrator::integrateProjective (voxgraph_amd/cpp/gpu_pointcloud_integrator.h) from plain C++
// over a stand-in message, for tests/test_range_image_cpp.py.
//   range_image_smoke header   no device: the method compiles, the host-only calls answer, NULL handles are refused
//   range_image_smoke          one PointXYZRGB sweep of a box room integrated through the method into one layer and through
//                              the C ABI (decode, vgx_range_image_build, vgx_tsdf_integrate_range_image) into another: the
//                              same counts, the same layer
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_pointcloud_integrator.h"
#include "pointcloud2_standin.h"

namespace {
using standin::PointCloud2;
using standin::PointField;
using voxgraph_amd::GpuPointcloudIntegrator;

struct Quat {
  float w_, x_, y_, z_;
  float w() const { return w_; }
  float x() const { return x_; }
  float y() const { return y_; }
  float z() const { return z_; }
};
struct Transformation {
  Quat q;
  float p[3];
  const Quat& getRotation() const { return q; }
  const float* getPosition() const { return p; }
};

vgx_lidar_model make_model() {
  vgx_lidar_model m{};
  m.width = 96;
  m.height = 12;
  m.azimuth_first_rad = 3.1415927f;
  m.azimuth_clockwise = 1;
  m.elevation_first_rad = 0.33f;
  m.elevation_last_rad = -0.33f;
  return m;
}

// one return per pixel of the model in a room of 5 x 3.6 x 2 m whose +x wall lies 6 m away (beyond the rays' 4 m), a few
// pixels without a return, a zero-length point and a second return in one pixel
void make_sweep(const vgx_lidar_model& m, PointCloud2* msg) {
  const char* names[4] = {"x", "y", "z", "rgb"};
  for (uint32_t k = 0; k < 4; ++k) {
    PointField f;
    f.name = names[k];
    f.offset = 4 * k;
    f.datatype = PointField::FLOAT32;
    f.count = 1;
    msg->fields.push_back(f);
  }
  msg->point_step = 16;
  std::vector<float> pts;
  std::vector<uint32_t> col;
  auto add = [&](double x, double y, double z, uint32_t c) {
    pts.push_back((float)x);
    pts.push_back((float)y);
    pts.push_back((float)z);
    col.push_back(c);
  };
  const double lo[3] = {-2.0, -1.6, -0.9}, hi[3] = {6.0, 2.0, 1.1};
  for (int v = 0; v < m.height; ++v)
    for (int u = 0; u < m.width; ++u) {
      if ((u * 7 + v * 3) % 29 == 0) continue;
      const double az = m.azimuth_first_rad - (u + 0.2) * 6.283185307179586 / m.width;
      const double el = m.elevation_first_rad + (v + 0.1) * (m.elevation_last_rad - m.elevation_first_rad) / (m.height - 1);
      const double d[3] = {std::cos(el) * std::cos(az), std::cos(el) * std::sin(az), std::sin(el)};
      double t = 1e9;
      for (int a = 0; a < 3; ++a) {
        if (d[a] > 1e-12) t = std::fmin(t, hi[a] / d[a]);
        if (d[a] < -1e-12) t = std::fmin(t, lo[a] / d[a]);
      }
      add(d[0] * t, d[1] * t, d[2] * t, 0xff000000u | (uint32_t)(u * 2) << 16 | (uint32_t)(v * 20) << 8 | (uint32_t)(u + v));
    }
  add(0.0, 0.0, 0.0, 0xffffffffu);
  add(pts[0] * 0.5, pts[1] * 0.5, pts[2] * 0.5, 0xff00ff00u);
  msg->width = (uint32_t)col.size();
  msg->height = 1;
  msg->row_step = msg->width * msg->point_step;
  msg->data.resize((size_t)msg->row_step);
  for (size_t i = 0; i < col.size(); ++i) {
    std::memcpy(&msg->data[16 * i], &pts[3 * i], 12);
    std::memcpy(&msg->data[16 * i + 12], &col[i], 4);
  }
}

struct Downloaded {
  int32_t nb = 0;
  std::vector<int32_t> bi;
  std::vector<float> dist, weight;
  std::vector<uint8_t> rgba;
  bool operator==(const Downloaded& o) const {
    return nb == o.nb && bi == o.bi && rgba == o.rgba && dist.size() == o.dist.size() &&
           std::memcmp(dist.data(), o.dist.data(), 4 * dist.size()) == 0 && std::memcmp(weight.data(), o.weight.data(), 4 * weight.size()) == 0;
  }
};
bool download(voxgraph_amd::GpuTsdfLayer& layer, int vps, Downloaded* d) {
  d->nb = layer.getNumberOfAllocatedBlocks();
  const size_t vox = (size_t)vps * vps * vps;
  d->bi.resize(3 * (size_t)d->nb);
  d->dist.resize(d->nb * vox);
  d->weight.resize(d->nb * vox);
  d->rgba.resize(4 * d->nb * vox);
  return vgx_tsdf_layer_download(layer.handle(), d->bi.data(), d->dist.data(), d->weight.data(), d->rgba.data()) == VGX_OK;
}
}  // namespace

int main(int argc, char** argv) {
  const vgx_lidar_model model = make_model();
  PointCloud2 msg;
  make_sweep(model, &msg);
  const Transformation pose{{0.98006658f, 0.0f, 0.0f, 0.19866933f}, {-3.2f, 0.4f, 1.1f}};
  const float T[7] = {pose.q.w_, pose.q.x_, pose.q.y_, pose.q.z_, pose.p[0], pose.p[1], pose.p[2]};
  if (argc == 2 && std::strcmp(argv[1], "header") == 0) {
    vgx_lidar_model bad = model;
    bad.height = 1;
    if (vgx_range_image_check(&model) != VGX_OK || vgx_range_image_check(&bad) != VGX_ERR_UNSUPPORTED) return 10;
    int32_t u = -1, v = -1;
    if (vgx_range_image_pixel(&model, -1.0f, 0.0f, 0.0f, &u, &v) != VGX_OK || u != 0 || v < 5 || v > 6) return 11;
    if (std::fabs(vgx_atan2_rule(1.0f, 1.0f) - 0.78539816f) > VGX_ATAN2_RULE_MAX_ERROR) return 12;
    vgx_range_image_counts none{};
    vgx_tsdf_config cfg;
    vgx_tsdf_config_default(&cfg);
    int32_t lo[3], hi[3];
    if (vgx_tsdf_range_image_box(&model, &none, &cfg, T, 0.1f, 8, lo, hi) != VGX_OK || !(lo[0] < hi[0])) return 13;
    if (vgx_tsdf_integrate_range_image(nullptr, T, nullptr, nullptr) != VGX_ERR_INVALID) return 14;
    if (vgx_range_image_build(nullptr, &model, nullptr, nullptr) != VGX_ERR_INVALID) return 15;
    const vgx_scan_layout l = GpuPointcloudIntegrator::layoutOf(msg);
    if (l.color_kind != VGX_SCAN_COLOR_RGB || l.color_offset != 12) return 16;
    printf("RANGE_IMAGE_HEADER_OK\n");
    return 0;
  }
  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  const float vs = 0.1f;
  const int vps = 8;
  try {
    voxgraph_amd::GpuFastTsdfIntegrator::Config cfg = voxgraph_amd::GpuFastTsdfIntegrator::defaultConfig();
    cfg.default_truncation_distance = 0.3f;
    cfg.max_ray_length_m = 4.0f;
    voxgraph_amd::GpuTsdfLayer by_method(ctx, vs, vps), by_abi(ctx, vs, vps);
    GpuPointcloudIntegrator integrator(ctx);
    integrator.setTsdfIntegratorConfig(cfg);
    bool refused = false;
    try {
      integrator.integrateProjective(pose, msg, model, nullptr);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    if (!refused) return 5;
    vgx_projective_counts a{}, b{};
    integrator.integrateProjective(pose, msg, model, &by_method, &a);
    integrator.integrateProjective(pose, msg, model, &by_method);  // queued
    vgx_range_image_counts ia{}, ib{};
    if (vgx_range_image_stats(integrator.rangeImage(), &ia, nullptr) != VGX_OK) return 6;

    voxgraph_amd::GpuFastTsdfIntegrator direct(ctx, cfg, &by_abi);
    vgx_scan scan = nullptr;
    vgx_range_image image = nullptr;
    if (vgx_scan_create(ctx, &scan) != VGX_OK || vgx_range_image_create(ctx, &image) != VGX_OK) return 6;
    const vgx_scan_layout l = GpuPointcloudIntegrator::layoutOf(msg);
    vgx_scan_config sc;
    vgx_scan_config_default(&sc);
    for (int k = 0; k < 2; ++k) {
      if (vgx_scan_decode_msg(scan, &l, &sc, msg.data.data(), (int64_t)msg.data.size()) != VGX_OK) return 6;
      if (vgx_range_image_build(image, &model, scan, k == 0 ? &ib : nullptr) != VGX_OK) return 6;
      if (vgx_tsdf_integrate_range_image(direct.handle(), T, image, k == 0 ? &b : nullptr) != VGX_OK) return 6;
    }
    if (std::memcmp(&a, &b, sizeof(a)) != 0 || a.n_updates < 1000 || a.n_new_blocks < 5 || a.n_carved < 100 || a.n_cleared < 100 ||
        ia.n_filled != ib.n_filled || ia.n_collided != 1 || ia.n_rejected_range != 1 || ia.n_points != (int64_t)msg.width) {
      fprintf(stderr, "counts: %lld %lld %lld %lld %lld; image %lld %lld %lld\n", (long long)a.n_candidate_blocks,
              (long long)a.n_new_blocks, (long long)a.n_updates, (long long)a.n_carved, (long long)a.n_cleared, (long long)ia.n_filled,
              (long long)ia.n_collided, (long long)ia.n_rejected_range);
      return 7;
    }
    Downloaded x, y;
    if (!download(by_method, vps, &x) || !download(by_abi, vps, &y)) return 8;
    if (!(x == y) || x.nb != (int32_t)a.n_new_blocks) return 9;
    vgx_range_image_destroy(image);
    vgx_scan_destroy(scan);
    printf("RANGE_IMAGE_SMOKE_OK blocks %d updates %lld\n", x.nb, (long long)a.n_updates);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  vgx_ctx_destroy(ctx);
  return 0;
}
