// voxgraph_amd::GpuDepthImageIntegrator::integrateProjective (voxgraph_amd/cpp/gpu_depth_image_integrator.h) from plain C++
// over stand-in messages, for tests/test_projective_cpp.py.
//   projective_smoke header   no device: the method compiles, a NULL layer and a foreign encoding are refused
//   projective_smoke          one 16UC1 frame with an RGB8 image integrated through the method into one layer and through
//                             the C ABI (vgx_tsdf_integrate_depth_image) into another: the same counts, the same layer
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_depth_image_integrator.h"
#include "image_standin.h"

namespace {
using standin::CameraInfo;
using standin::Image;
using voxgraph_amd::GpuDepthImageIntegrator;

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

// a wall at 1.5 m whose right part is 5.5 m away (beyond the rays' 4 m), a hole, rows padded by two bytes
void make_frame(Image* depth, Image* colour, CameraInfo* info) {
  const uint32_t w = 40, h = 30;
  depth->width = colour->width = w;
  depth->height = colour->height = h;
  depth->encoding = "16UC1";
  depth->step = 2 * w + 2;
  depth->data.assign((size_t)depth->step * h, 0);
  colour->encoding = "rgb8";
  colour->step = 3 * w + 1;
  colour->data.assign((size_t)colour->step * h, 0);
  for (uint32_t v = 0; v < h; ++v)
    for (uint32_t u = 0; u < w; ++u) {
      uint16_t mm = u < 28 ? (uint16_t)(1500 + 3 * u + 2 * v) : 5500;
      if (u > 10 && u < 14 && v > 20) mm = 0;
      std::memcpy(&depth->data[(size_t)v * depth->step + 2 * u], &mm, 2);
      uint8_t* c = &colour->data[(size_t)v * colour->step + 3 * u];
      c[0] = (uint8_t)(5 * u);
      c[1] = (uint8_t)(7 * v);
      c[2] = (uint8_t)(u * v);
    }
  info->K = {35.0, 0.0, 19.5, 0.0, 35.0, 14.5, 0.0, 0.0, 1.0};
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
  Image depth, colour;
  CameraInfo info;
  make_frame(&depth, &colour, &info);
  const Transformation pose{{0.98006658f, 0.0f, 0.19866933f, 0.0f}, {-3.2f, 0.4f, 1.1f}};
  if (argc == 2 && std::strcmp(argv[1], "header") == 0) {
    Image bad = depth;
    bad.encoding = "8UC1";
    bool refused = false;
    try {
      GpuDepthImageIntegrator::layoutOf(bad, &colour);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    const vgx_depth_image_layout l = GpuDepthImageIntegrator::layoutOf(depth, &colour);
    vgx_depth_camera cam;
    vgx_depth_camera_default(&cam);
    cam = GpuDepthImageIntegrator::cameraFrom(cam, info);
    vgx_tsdf_config cfg;
    vgx_tsdf_config_default(&cfg);
    const float T[7] = {pose.q.w_, pose.q.x_, pose.q.y_, pose.q.z_, pose.p[0], pose.p[1], pose.p[2]};
    int32_t lo[3], hi[3];
    if (!refused || vgx_tsdf_projective_box(&l, &cam, &cfg, T, 0.1f, 8, lo, hi) != VGX_OK || !(lo[0] < hi[0])) return 10;
    if (vgx_tsdf_integrate_depth_image(nullptr, T, &l, &cam, depth.data.data(), (int64_t)depth.data.size(), colour.data.data(),
                                       (int64_t)colour.data.size(), nullptr) != VGX_ERR_INVALID)
      return 11;
    printf("PROJECTIVE_HEADER_OK\n");
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
    GpuDepthImageIntegrator integrator(ctx);
    integrator.setTsdfIntegratorConfig(cfg);
    bool refused = false;
    try {
      integrator.integrateProjective(pose, depth, info, &colour, nullptr);
    } catch (const std::invalid_argument&) {
      refused = true;
    }
    if (!refused) return 5;
    vgx_projective_counts a{}, b{};
    integrator.integrateProjective(pose, depth, info, &colour, &by_method, &a);
    integrator.integrateProjective(pose, depth, info, &colour, &by_method);  // queued
    integrator.integrateProjective(pose, depth, info, &by_method);           // without colours, queued

    voxgraph_amd::GpuFastTsdfIntegrator direct(ctx, cfg, &by_abi);
    const vgx_depth_image_layout l = GpuDepthImageIntegrator::layoutOf(depth, &colour);
    const vgx_depth_image_layout plain = GpuDepthImageIntegrator::layoutOf(depth, static_cast<const Image*>(nullptr));
    const vgx_depth_camera cam = integrator.cameraOf(info);
    const float T[7] = {pose.q.w_, pose.q.x_, pose.q.y_, pose.q.z_, pose.p[0], pose.p[1], pose.p[2]};
    for (int k = 0; k < 3; ++k)
      if (vgx_tsdf_integrate_depth_image(direct.handle(), T, k < 2 ? &l : &plain, &cam, depth.data.data(), (int64_t)depth.data.size(),
                                         k < 2 ? colour.data.data() : nullptr, k < 2 ? (int64_t)colour.data.size() : 0,
                                         k == 0 ? &b : nullptr) != VGX_OK)
        return 6;
    if (std::memcmp(&a, &b, sizeof(a)) != 0 || a.n_updates < 1000 || a.n_new_blocks < 5 || a.n_carved < 100 || a.n_cleared < 100) {
      fprintf(stderr, "counts: %lld %lld %lld %lld %lld\n", (long long)a.n_candidate_blocks, (long long)a.n_new_blocks,
              (long long)a.n_updates, (long long)a.n_carved, (long long)a.n_cleared);
      return 7;
    }
    Downloaded x, y;
    if (!download(by_method, vps, &x) || !download(by_abi, vps, &y)) return 8;
    if (!(x == y) || x.nb != (int32_t)a.n_new_blocks) return 9;
    printf("PROJECTIVE_SMOKE_OK blocks %d updates %lld\n", x.nb, (long long)a.n_updates);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  vgx_ctx_destroy(ctx);
  return 0;
}
