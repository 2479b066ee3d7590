// voxgraph_amd::GpuPointcloudIntegrator::integrateProjective for a beam table and sortedBeamTable
// (voxgraph_amd/cpp/gpu_pointcloud_integrator.h) from plain C++ over a stand-in message, for tests/test_beam_table_cpp.py.
//   beam_table_smoke header   no device: the overload compiles, the sort helper sorts a table in laser order and returns
//                             the permutation, the host-only calls answer, NULL handles are refused
//   beam_table_smoke          one PointXYZRGB sweep of a box room by a 12-beam sensor with azimuth offsets, integrated
//                             through the method into one layer and through the C ABI (decode, vgx_range_image_build_beams,
//                             vgx_tsdf_integrate_range_image) into another: the same counts, the same layer
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

// 12 beams in laser order: the lower block's six, then the upper block's, each block firing outside in; dense near the
// horizon, sparse at the edges
const float kLaserElevation[12] = {-0.33f, -0.02f, -0.21f, -0.05f, -0.12f, -0.08f, 0.33f, 0.01f, 0.22f, 0.04f, 0.13f, 0.07f};
const float kLaserOffset[12] = {0.05f, -0.05f, 0.03f, -0.03f, 0.01f, -0.01f, 0.05f, -0.05f, 0.03f, -0.03f, 0.01f, -0.01f};

// one return per pixel of the model (sorted rows) in a room of 5 x 3.6 x 2 m whose +x wall lies 6 m away (beyond the rays' 4 m), a few
// pixels without a return, a zero-length point and a second return in one pixel
void make_sweep(const vgx_lidar_beam_model& m, PointCloud2* msg) {
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
      const double az = m.azimuth_first_rad + m.row_azimuth_offset_rad[v] - (u + 0.2) * 6.283185307179586 / m.width;
      const double el = m.row_elevation_rad[v] + 0.002;
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
  const GpuPointcloudIntegrator::SortedBeamTable table = GpuPointcloudIntegrator::sortedBeamTable(kLaserElevation, kLaserOffset, 12);
  const vgx_lidar_beam_model model = table.view(96, 3.1415927f, 1, INFINITY);
  PointCloud2 msg;
  make_sweep(model, &msg);
  const Transformation pose{{0.98006658f, 0.0f, 0.0f, 0.19866933f}, {-3.2f, 0.4f, 1.1f}};
  const float T[7] = {pose.q.w_, pose.q.x_, pose.q.y_, pose.q.z_, pose.p[0], pose.p[1], pose.p[2]};
  if (argc == 2 && std::strcmp(argv[1], "header") == 0) {
    // sorted ascending, the permutation says which laser a row is, and the offsets moved with their rows
    const int32_t want[12] = {0, 2, 4, 5, 3, 1, 7, 9, 11, 10, 8, 6};
    for (int k = 0; k < 12; ++k) {
      if (table.order[k] != want[k] || table.row_elevation_rad[k] != kLaserElevation[want[k]] ||
          table.row_azimuth_offset_rad[k] != kLaserOffset[want[k]])
        return 10;
      if (k > 0 && !(table.row_elevation_rad[k] > table.row_elevation_rad[k - 1])) return 10;
    }
    if (GpuPointcloudIntegrator::sortedBeamTable(kLaserElevation, nullptr, 12).view(96, 0.0f, 0, 0.1f).row_azimuth_offset_rad != nullptr) return 10;
    vgx_lidar_beam_model laser = model;  // the laser order itself is not monotone: refused
    laser.row_elevation_rad = kLaserElevation;
    if (vgx_range_image_check_beams(&model) != VGX_OK || vgx_range_image_check_beams(&laser) != VGX_ERR_INVALID) return 10;
    int32_t u = -1, v = -1;
    // row 5 is laser 1 (elevation -0.02, offset -0.05): column 0 looks backwards, -x lies 0.05 rad = 0.76 columns on
    if (vgx_range_image_pixel_beams(&model, -1.0f, 0.0f, -0.02f, &u, &v) != VGX_OK || u != 95 || v != 5) return 11;
    if (vgx_range_image_pixel_beams(&model, 0.0f, 0.0f, 1.0f, &u, &v) != VGX_OK || u != -1 || v != -1) return 11;
    std::vector<float> dirs(3 * 96 * 12);
    if (vgx_view_rays_lidar_beams(&model, dirs.data()) != VGX_OK) return 12;
    const float* d = &dirs[3 * (7 * 96 + 40)];
    if (vgx_range_image_pixel_beams(&model, d[0], d[1], d[2], &u, &v) != VGX_OK || u != 40 || v != 7) return 12;
    vgx_range_image_counts none{};
    vgx_tsdf_config cfg;
    vgx_tsdf_config_default(&cfg);
    int32_t lo[3], hi[3];
    if (vgx_tsdf_range_image_box_beams(&model, &none, &cfg, T, 0.1f, 8, lo, hi) != VGX_OK || !(lo[0] < hi[0])) return 13;
    if (vgx_range_image_build_beams(nullptr, &model, nullptr, nullptr) != VGX_ERR_INVALID) return 15;
    if (vgx_range_image_beams(nullptr, nullptr, nullptr, nullptr, nullptr) != VGX_ERR_INVALID) return 15;
    const vgx_scan_layout l = GpuPointcloudIntegrator::layoutOf(msg);
    if (l.color_kind != VGX_SCAN_COLOR_RGB || l.color_offset != 12) return 16;
    printf("BEAM_TABLE_HEADER_OK\n");
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
      if (vgx_range_image_build_beams(image, &model, scan, k == 0 ? &ib : nullptr) != VGX_OK) return 6;
      if (vgx_tsdf_integrate_range_image(direct.handle(), T, image, k == 0 ? &b : nullptr) != VGX_OK) return 6;
    }
    if (std::memcmp(&a, &b, sizeof(a)) != 0 || a.n_updates < 1000 || a.n_new_blocks < 5 || a.n_carved < 100 || a.n_cleared < 100 ||
        ia.n_filled != ib.n_filled || ia.n_collided != 1 || ia.n_rejected_range != 1 || ia.n_points != (int64_t)msg.width) {
      fprintf(stderr, "counts: %lld %lld %lld %lld %lld; image %lld %lld %lld\n", (long long)a.n_candidate_blocks,
              (long long)a.n_new_blocks, (long long)a.n_updates, (long long)a.n_carved, (long long)a.n_cleared, (long long)ia.n_filled,
              (long long)ia.n_collided, (long long)ia.n_rejected_range);
      return 7;
    }
    int32_t is_table = 0;
    float el[12], off[12], limit = 0.0f;
    if (vgx_range_image_beams(integrator.rangeImage(), &is_table, el, off, &limit) != VGX_OK || is_table != 1 || !std::isinf(limit) ||
        std::memcmp(el, table.row_elevation_rad.data(), sizeof(el)) != 0 || std::memcmp(off, table.row_azimuth_offset_rad.data(), sizeof(off)) != 0)
      return 7;
    Downloaded x, y;
    if (!download(by_method, vps, &x) || !download(by_abi, vps, &y)) return 8;
    if (!(x == y) || x.nb != (int32_t)a.n_new_blocks) return 9;
    vgx_range_image_destroy(image);
    vgx_scan_destroy(scan);
    printf("BEAM_TABLE_SMOKE_OK blocks %d updates %lld\n", x.nb, (long long)a.n_updates);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  vgx_ctx_destroy(ctx);
  return 0;
}
