// voxgraph::PointcloudIntegrator's mirror (voxgraph_amd/cpp/gpu_pointcloud_integrator.h) from plain C++ over stand-in
// messages (tests/cpp/pointcloud2_standin.h), for tests/test_scan_msg_cpp.py.
//   scan_msg_smoke layout          no device: the field detection and its refusals
//   scan_msg_smoke IN OUT          integrates the messages of IN into one layer and writes the layer to OUT
// IN: int32 n_msgs, vps, deterministic; f32 voxel_size; per message: f32 T[7]; u32 width, height, point_step, row_step,
//     is_bigendian, n_fields; per field: u32 name length, the name, u32 offset, datatype, count; u64 n_bytes; the bytes
// OUT: int32 n_blocks; int32 block_index [n][3]; f32 distance, weight [n][vps^3]; u8 rgba [n][vps^3][4]; int64 points
//     integrated per message; int32 cloud width given to the integrator per message
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_pointcloud_integrator.h"
#include "pointcloud2_standin.h"

namespace {
using standin::PointCloud2;
using standin::PointField;
using voxgraph_amd::GpuPointcloudIntegrator;

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}

PointField field(const char* name, uint32_t offset, uint8_t datatype, uint32_t count = 1) {
  PointField f;
  f.name = name;
  f.offset = offset;
  f.datatype = datatype;
  f.count = count;
  return f;
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

int layout_checks() {
  PointCloud2 m;
  m.width = 5;
  m.height = 2;
  m.point_step = 32;
  m.row_step = 200;
  m.fields = {field("x", 0, PointField::FLOAT32), field("y", 4, PointField::FLOAT32), field("z", 8, PointField::FLOAT32)};
  vgx_scan_layout l = GpuPointcloudIntegrator::layoutOf(m);
  if (l.width != 5 || l.height != 2 || l.point_step != 32 || l.row_step != 200 || l.offset_x != 0 || l.offset_y != 4 ||
      l.offset_z != 8 || l.color_kind != VGX_SCAN_COLOR_NONE || l.is_bigendian != 0)
    return 10;
  if (vgx_scan_layout_check(&l, 400) != VGX_OK || vgx_scan_layout_check(&l, 359) != VGX_ERR_INVALID) return 11;
  m.fields.push_back(field("intensity", 16, PointField::FLOAT32));
  l = GpuPointcloudIntegrator::layoutOf(m);
  if (l.color_kind != VGX_SCAN_COLOR_INTENSITY || l.color_offset != 16) return 12;
  // a field named rgb wins wherever it stands, and its datatype is not looked at (pointcloud_integrator.cpp:36-39)
  m.fields.insert(m.fields.begin(), field("rgb", 20, PointField::UINT32));
  l = GpuPointcloudIntegrator::layoutOf(m);
  if (l.color_kind != VGX_SCAN_COLOR_RGB || l.color_offset != 20) return 13;
  m.fields.push_back(field("ring", 24, PointField::UINT16));  // other fields are ignored
  l = GpuPointcloudIntegrator::layoutOf(m);
  if (l.color_kind != VGX_SCAN_COLOR_RGB || l.color_offset != 20 || l.offset_z != 8) return 14;
  m.is_bigendian = 1;
  l = GpuPointcloudIntegrator::layoutOf(m);
  if (l.is_bigendian != 1 || vgx_scan_layout_check(&l, 400) != VGX_ERR_UNSUPPORTED) return 15;
  // refusals: coordinates that are not one FLOAT32, an intensity that is not FLOAT32, a missing coordinate
  PointCloud2 bad = m;
  bad.fields = {field("x", 0, PointField::FLOAT64), field("y", 8, PointField::FLOAT64), field("z", 16, PointField::FLOAT64)};
  if (!throws_invalid([&] { GpuPointcloudIntegrator::layoutOf(bad); })) return 16;
  bad.fields = {field("x", 0, PointField::FLOAT32), field("y", 4, PointField::FLOAT32), field("z", 8, PointField::INT32)};
  if (!throws_invalid([&] { GpuPointcloudIntegrator::layoutOf(bad); })) return 17;
  bad.fields = {field("x", 0, PointField::FLOAT32, 3), field("y", 4, PointField::FLOAT32), field("z", 8, PointField::FLOAT32)};
  if (!throws_invalid([&] { GpuPointcloudIntegrator::layoutOf(bad); })) return 18;
  bad.fields = {field("x", 0, PointField::FLOAT32), field("y", 4, PointField::FLOAT32), field("z", 8, PointField::FLOAT32),
                field("intensity", 12, PointField::UINT16)};
  if (!throws_invalid([&] { GpuPointcloudIntegrator::layoutOf(bad); })) return 19;
  bad.fields = {field("x", 0, PointField::FLOAT32), field("z", 8, PointField::FLOAT32)};
  if (!throws_invalid([&] { GpuPointcloudIntegrator::layoutOf(bad); })) return 20;
  printf("SCAN_MSG_LAYOUT_OK\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "layout") == 0) return layout_checks();
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t n_msgs = 0, vps = 0, deterministic = 0;
  float vs = 0;
  if (!rd(in, &n_msgs, 1) || !rd(in, &vps, 1) || !rd(in, &deterministic, 1) || !rd(in, &vs, 1)) return 3;
  std::vector<PointCloud2> msgs((size_t)n_msgs);
  std::vector<Transformation> poses((size_t)n_msgs);
  for (int k = 0; k < n_msgs; ++k) {
    PointCloud2& m = msgs[k];
    float T[7];
    uint32_t h[6];
    if (!rd(in, T, 7) || !rd(in, h, 6)) return 3;
    poses[k] = Transformation{{T[0], T[1], T[2], T[3]}, {T[4], T[5], T[6]}};
    m.width = h[0];
    m.height = h[1];
    m.point_step = h[2];
    m.row_step = h[3];
    m.is_bigendian = (uint8_t)h[4];
    for (uint32_t d = 0; d < h[5]; ++d) {
      uint32_t len = 0, f[3];
      if (!rd(in, &len, 1) || len > 64) return 3;
      std::string name(len, ' ');
      if (!rd(in, &name[0], len) || !rd(in, f, 3)) return 3;
      m.fields.push_back(field(name.c_str(), f[0], (uint8_t)f[1], f[2]));
    }
    uint64_t n_bytes = 0;
    if (!rd(in, &n_bytes, 1)) return 3;
    m.data.resize((size_t)n_bytes);
    if (!rd(in, m.data.data(), m.data.size())) return 3;
  }
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  std::vector<int64_t> counts;
  std::vector<int32_t> widths;
  int32_t nb = 0;
  std::vector<int32_t> bi;
  std::vector<float> dist, weight;
  std::vector<uint8_t> rgba;
  try {
    voxgraph_amd::GpuTsdfLayer layer(ctx, vs, vps);
    GpuPointcloudIntegrator integrator(ctx);
    voxgraph_amd::GpuFastTsdfIntegrator::Config cfg = voxgraph_amd::GpuFastTsdfIntegrator::defaultConfig();
    cfg.default_truncation_distance = 0.6f;  // voxgraph_mapper.yaml:21-28
    cfg.max_ray_length_m = 16.0f;
    cfg.use_const_weight = 1;
    cfg.use_weight_dropoff = 1;
    cfg.use_sparsity_compensation_factor = 1;
    cfg.sparsity_compensation_factor = 20.0f;
    cfg.deterministic = deterministic;
    integrator.setTsdfIntegratorConfig(cfg);
    for (int k = 0; k < n_msgs; ++k) {
      integrator.integratePointcloud(msgs[k], poses[k], &layer);
      counts.push_back(integrator.lastPointcloudSize());
      widths.push_back(integrator.lastCloudWidth());
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
  fwrite(widths.data(), 4, widths.size(), out);
  fclose(out);
  printf("SCAN_MSG_SMOKE_OK\n");
  return 0;
}
