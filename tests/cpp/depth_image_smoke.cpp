// voxgraph_amd::GpuDepthImageIntegrator (voxgraph_amd/cpp/gpu_depth_image_integrator.h) from plain C++ over stand-in
// messages, for tests/test_depth_image_cpp.py.
//   depth_image_smoke encodings   no device: the encodings resolved, the layout and camera formed, the refusals
//   depth_image_smoke IN OUT      integrates the frames of IN into one layer and writes the layer and the counts to OUT
// IN: i32 n_frames, voxels per side; f32 voxel size; f32 depth_unit_m, min_depth_m, max_depth_m; i32 stride_u, stride_v;
//     per frame: f32 T_submap_camera[7]; f64 K[9]; the depth image; u32 has_colour; the colour image if so.  An image: u32
//     width, height, step, is_bigendian, encoding length; the encoding; u64 n_bytes; the bytes.
// OUT: i32 blocks; i32 block_index[blocks][3]; f32 distance, weight [blocks][vps^3]; u8 rgba[blocks][vps^3][4];
//     per frame: i64 points, dropped, candidates, invalid, out of range, overflowed
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_depth_image_integrator.h"
#include "image_standin.h"

namespace {
using standin::CameraInfo;
using standin::Image;
using voxgraph_amd::GpuDepthImageIntegrator;

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}

bool rd_image(FILE* f, Image* m) {
  uint32_t h[5];
  if (!rd(f, h, 5) || h[4] > 64) return false;
  m->width = h[0];
  m->height = h[1];
  m->step = h[2];
  m->is_bigendian = (uint8_t)h[3];
  m->encoding.assign(h[4], ' ');
  uint64_t n_bytes = 0;
  if (!rd(f, &m->encoding[0], h[4]) || !rd(f, &n_bytes, 1)) return false;
  m->data.resize((size_t)n_bytes);
  return rd(f, m->data.data(), m->data.size());
}

template <class Fn>
bool throws_invalid(Fn fn) {
  try {
    fn();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

// kindr's transformation, as far as the mirror reads it
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

int encoding_checks() {
  Image d;
  d.width = 6;
  d.height = 4;
  d.step = 14;
  const char* depth_names[3] = {"16UC1", "mono16", "32FC1"};
  const int32_t depth_kinds[3] = {VGX_DEPTH_16UC1, VGX_DEPTH_16UC1, VGX_DEPTH_32FC1};
  for (int k = 0; k < 3; ++k) {
    d.encoding = depth_names[k];
    if (GpuDepthImageIntegrator::depthEncodingOf(d) != depth_kinds[k]) return 10;
  }
  Image c;
  c.width = 6;
  c.height = 4;
  c.step = 25;
  const char* colour_names[5] = {"rgb8", "bgr8", "rgba8", "bgra8", "mono8"};
  const int32_t colour_kinds[5] = {VGX_IMAGE_COLOR_RGB8, VGX_IMAGE_COLOR_BGR8, VGX_IMAGE_COLOR_RGBA8, VGX_IMAGE_COLOR_BGRA8,
                                   VGX_IMAGE_COLOR_MONO8};
  for (int k = 0; k < 5; ++k) {
    c.encoding = colour_names[k];
    if (GpuDepthImageIntegrator::colorKindOf(c) != colour_kinds[k]) return 11;
  }
  d.encoding = "16UC1";
  c.encoding = "bgr8";
  vgx_depth_image_layout l = GpuDepthImageIntegrator::layoutOf(d, static_cast<const Image*>(nullptr));
  if (l.width != 6 || l.height != 4 || l.row_step != 14 || l.encoding != VGX_DEPTH_16UC1 || l.is_bigendian != 0 ||
      l.color_kind != VGX_IMAGE_COLOR_NONE || l.color_row_step != 0)
    return 12;
  l = GpuDepthImageIntegrator::layoutOf(d, &c);
  if (l.color_kind != VGX_IMAGE_COLOR_BGR8 || l.color_row_step != 25) return 13;
  // refusals: encodings that are not in the lists (8- and 64-bit depth, a Bayer image), a colour image of another size
  Image bad = d;
  for (const char* e : {"8UC1", "64FC1", "32FC3", "rgb8", ""}) {
    bad.encoding = e;
    if (!throws_invalid([&] { GpuDepthImageIntegrator::depthEncodingOf(bad); })) return 14;
  }
  bad = c;
  for (const char* e : {"bayer_rggb8", "rgb16", "16UC1", "RGB8"}) {
    bad.encoding = e;
    if (!throws_invalid([&] { GpuDepthImageIntegrator::colorKindOf(bad); })) return 15;
  }
  bad = c;
  bad.width = 5;
  if (!throws_invalid([&] { GpuDepthImageIntegrator::layoutOf(d, &bad); })) return 16;
  bad = c;
  bad.height = 8;
  if (!throws_invalid([&] { GpuDepthImageIntegrator::layoutOf(d, &bad); })) return 17;
  // the camera: K's entries over the integrator's own fields, and what the host-only check makes of the two
  vgx_depth_camera own;
  vgx_depth_camera_default(&own);
  own.min_depth_m = 0.5f;
  own.stride_v = 2;
  CameraInfo info;
  info.K = {525.0, 0.0, 319.5, 0.0, 526.0, 239.5, 0.0, 0.0, 1.0};
  const vgx_depth_camera cam = GpuDepthImageIntegrator::cameraFrom(own, info);
  if (cam.fx != 525.0 || cam.fy != 526.0 || cam.cx != 319.5 || cam.cy != 239.5 || cam.min_depth_m != 0.5f || cam.stride_v != 2 ||
      cam.depth_unit_m != 0.001f)
    return 18;
  l = GpuDepthImageIntegrator::layoutOf(d, &c);
  if (vgx_depth_image_check(&l, &cam, 3 * 14 + 12, 3 * 25 + 18) != VGX_OK) return 19;
  if (vgx_depth_image_check(&l, &cam, 3 * 14 + 11, 3 * 25 + 18) != VGX_ERR_INVALID) return 20;
  if (vgx_depth_image_check(&l, &cam, 3 * 14 + 12, 3 * 25 + 17) != VGX_ERR_INVALID) return 21;
  d.is_bigendian = 1;
  l = GpuDepthImageIntegrator::layoutOf(d, &c);
  if (l.is_bigendian != 1 || vgx_depth_image_check(&l, &cam, 1000, 1000) != VGX_ERR_UNSUPPORTED) return 22;
  printf("DEPTH_IMAGE_ENCODINGS_OK\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "encodings") == 0) return encoding_checks();
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t n_frames = 0, vps = 0, strides[2] = {1, 1};
  float vs = 0, gate[3] = {0, 0, 0};
  if (!rd(in, &n_frames, 1) || !rd(in, &vps, 1) || !rd(in, &vs, 1) || !rd(in, gate, 3) || !rd(in, strides, 2)) return 3;
  std::vector<Image> depths((size_t)n_frames), colours((size_t)n_frames);
  std::vector<CameraInfo> infos((size_t)n_frames);
  std::vector<Transformation> poses((size_t)n_frames);
  std::vector<uint32_t> has_colour((size_t)n_frames);
  for (int k = 0; k < n_frames; ++k) {
    float T[7];
    if (!rd(in, T, 7) || !rd(in, infos[k].K.data(), 9) || !rd_image(in, &depths[k]) || !rd(in, &has_colour[k], 1)) return 3;
    poses[k] = Transformation{{T[0], T[1], T[2], T[3]}, {T[4], T[5], T[6]}};
    if (has_colour[k] && !rd_image(in, &colours[k])) return 3;
  }
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  std::vector<int64_t> counts;
  int32_t nb = 0;
  std::vector<int32_t> bi;
  std::vector<float> dist, weight;
  std::vector<uint8_t> rgba;
  try {
    voxgraph_amd::GpuTsdfLayer layer(ctx, vs, vps);
    GpuDepthImageIntegrator integrator(ctx);
    voxgraph_amd::GpuFastTsdfIntegrator::Config cfg = voxgraph_amd::GpuFastTsdfIntegrator::defaultConfig();
    cfg.default_truncation_distance = 0.6f;  // voxgraph_mapper.yaml:21-28
    cfg.max_ray_length_m = 16.0f;
    cfg.use_const_weight = 1;
    cfg.use_weight_dropoff = 1;
    cfg.use_sparsity_compensation_factor = 1;
    cfg.sparsity_compensation_factor = 20.0f;
    cfg.deterministic = 1;
    integrator.setTsdfIntegratorConfig(cfg);
    integrator.camera().depth_unit_m = gate[0];
    integrator.camera().min_depth_m = gate[1];
    integrator.camera().max_depth_m = gate[2];
    integrator.camera().stride_u = strides[0];
    integrator.camera().stride_v = strides[1];
    for (int k = 0; k < n_frames; ++k) {
      integrator.integrateDepthImage(poses[k], depths[k], infos[k], has_colour[k] ? &colours[k] : nullptr, &layer);
      int64_t c[6] = {0, 0, 0, 0, 0, 0};
      if (vgx_scan_stats(integrator.scan(), &c[0], &c[1]) != VGX_OK) return 6;
      if (vgx_scan_depth_stats(integrator.scan(), &c[2], &c[3], &c[4], &c[5]) != VGX_OK) return 6;
      if (integrator.lastPointcloudSize() != c[0]) return 6;
      counts.insert(counts.end(), c, c + 6);
    }
    nb = layer.getNumberOfAllocatedBlocks();
    const size_t vox = (size_t)vps * vps * vps;
    bi.resize(3 * (size_t)nb);
    dist.resize(nb * vox);
    weight.resize(nb * vox);
    rgba.resize(4 * nb * vox);
    if (vgx_tsdf_layer_download(layer.handle(), bi.data(), dist.data(), weight.data(), rgba.data()) != VGX_OK) return 6;
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  vgx_ctx_destroy(ctx);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 7;
  fwrite(&nb, 4, 1, out);
  fwrite(bi.data(), 4, bi.size(), out);
  fwrite(dist.data(), 4, dist.size(), out);
  fwrite(weight.data(), 4, weight.size(), out);
  fwrite(rgba.data(), 1, rgba.size(), out);
  fwrite(counts.data(), 8, counts.size(), out);
  fclose(out);
  printf("DEPTH_IMAGE_SMOKE_OK\n");
  return 0;
}
