// The undistorting path of voxgraph::PointcloudIntegrator's mirror (voxgraph_amd/cpp/gpu_pointcloud_integrator.h) from
// plain C++ over a stand-in message, for tests/test_scan_undistort_cpp.py.
//   scan_undistort_smoke fields     no device: timeFieldOf and its refusals
//   scan_undistort_smoke IN OUT     builds the track with GpuScanTrack, integrates the message undistorted and writes the
//                                   knots, the counters and the scan it decoded to OUT
// IN: u32 width, height, point_step, row_step, is_bigendian, n_fields; per field: u32 name length, the name, u32 offset,
//     datatype, count; u64 n_bytes; the bytes; f64 stamp; f64 T_fixed_sensor_ref[7]; f32 T_submap_sensor_ref[7];
//     i32 n_samples; per sample: f64 t, f64 T_fixed_sensor[7]
// OUT: i32 K; f64 knot_time[K]; f32 knot_T[K][7]; i64 points, dropped, bad_time, overflowed, clamped; f32 points[n][3];
//     u8 rgba[n][4]; i32 blocks in the layer
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_pointcloud_integrator.h"
#include "pointcloud2_standin.h"

namespace {
using standin::PointCloud2;
using standin::PointField;
using voxgraph_amd::GpuPointcloudIntegrator;
using voxgraph_amd::GpuScanTrack;

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
// ... and its double-precision form (the odometry's poses)
struct QuatD {
  double w_, x_, y_, z_;
  double w() const { return w_; }
  double x() const { return x_; }
  double y() const { return y_; }
  double z() const { return z_; }
};
struct TransformationD {
  QuatD q;
  double p[3];
  const QuatD& getRotation() const { return q; }
  const double* getPosition() const { return p; }
};
TransformationD transformation_d(const double* T) { return TransformationD{{T[0], T[1], T[2], T[3]}, {T[4], T[5], T[6]}}; }

int field_checks() {
  PointCloud2 m;
  m.point_step = 48;
  m.fields = {field("x", 0, PointField::FLOAT32), field("y", 4, PointField::FLOAT32), field("z", 8, PointField::FLOAT32),
              field("timestamp", 32, PointField::FLOAT64), field("time", 28, PointField::FLOAT32), field("t", 20, PointField::UINT32)};
  // "t" wins wherever it stands, then "time", then "timestamp"
  vgx_scan_time_field f = GpuPointcloudIntegrator::timeFieldOf(m, 100.5);
  if (f.kind != VGX_SCAN_TIME_UINT32 || f.offset != 20 || f.scale != 1e-9 || f.offset_s != 0.0) return 10;
  m.fields.pop_back();
  f = GpuPointcloudIntegrator::timeFieldOf(m, 100.5);
  if (f.kind != VGX_SCAN_TIME_FLOAT32 || f.offset != 28 || f.scale != 1.0 || f.offset_s != 0.0) return 11;
  m.fields.pop_back();
  f = GpuPointcloudIntegrator::timeFieldOf(m, 100.5);
  if (f.kind != VGX_SCAN_TIME_FLOAT64 || f.offset != 32 || f.scale != 1.0 || f.offset_s != -100.5) return 12;
  // a "t" of another type or count is not the rule's field: the next rule's field is taken
  m.fields.push_back(field("t", 20, PointField::FLOAT32));
  m.fields.push_back(field("time", 24, PointField::FLOAT32, 2));
  f = GpuPointcloudIntegrator::timeFieldOf(m, 0.0);
  if (f.kind != VGX_SCAN_TIME_FLOAT64 || f.offset != 32) return 13;
  // refusals: no time field at all; only fields of the wrong type
  PointCloud2 bad = m;
  bad.fields = {field("x", 0, PointField::FLOAT32), field("y", 4, PointField::FLOAT32), field("z", 8, PointField::FLOAT32)};
  if (!throws_invalid([&] { GpuPointcloudIntegrator::timeFieldOf(bad, 0.0); })) return 14;
  bad.fields.push_back(field("t", 20, PointField::INT32));
  bad.fields.push_back(field("time", 24, PointField::FLOAT64));
  bad.fields.push_back(field("timestamp", 32, PointField::FLOAT32));
  bad.fields.push_back(field("stamp", 40, PointField::FLOAT64));
  if (!throws_invalid([&] { GpuPointcloudIntegrator::timeFieldOf(bad, 0.0); })) return 15;
  // the host-only check takes what timeFieldOf and GpuScanTrack make
  GpuScanTrack track;
  const double a[7] = {1, 0, 0, 0, 0, 0, 0}, b[7] = {1, 0, 0, 0, 1, 0, 0};
  track.add7(5.0, a);
  track.add7(5.1, b);
  const GpuScanTrack::Knots knots = track.relativeTo7(b, 5.0);
  if (knots.knot_time.size() != 2 || knots.knot_time[0] != 0.0 || knots.knot_T[4] != -1.0f || knots.knot_T[7 + 4] != 0.0f) return 16;
  vgx_scan_layout l{};
  l.width = 2;
  l.height = 1;
  l.point_step = 48;
  l.row_step = 96;
  l.offset_y = 4;
  l.offset_z = 8;
  const vgx_scan_track view = knots.view();
  if (vgx_scan_undistort_check(&l, &f, &view, 96) != VGX_OK || vgx_scan_undistort_check(&l, &f, &view, 95) != VGX_ERR_INVALID) return 17;
  f.offset = 41;
  if (vgx_scan_undistort_check(&l, &f, &view, 96) != VGX_ERR_INVALID) return 18;
  printf("SCAN_UNDISTORT_FIELDS_OK\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "fields") == 0) return field_checks();
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  PointCloud2 m;
  uint32_t h[6];
  if (!rd(in, h, 6)) return 3;
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
  double stamp = 0, ref[7];
  float Ts[7];
  int32_t n_samples = 0;
  if (!rd(in, m.data.data(), m.data.size()) || !rd(in, &stamp, 1) || !rd(in, ref, 7) || !rd(in, Ts, 7) || !rd(in, &n_samples, 1)) return 3;
  GpuScanTrack track;
  for (int k = 0; k < n_samples; ++k) {
    double s[8];
    if (!rd(in, s, 8)) return 3;
    track.add(s[0], transformation_d(s + 1));
  }
  fclose(in);
  const GpuScanTrack::Knots knots = track.relativeTo(transformation_d(ref), stamp);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  int64_t counts[5] = {0, 0, 0, 0, 0};
  std::vector<float> points;
  std::vector<uint8_t> rgba;
  int32_t blocks = 0;
  try {
    voxgraph_amd::GpuTsdfLayer layer(ctx, 0.2f, 16);
    GpuPointcloudIntegrator integrator(ctx);
    const Transformation T{{Ts[0], Ts[1], Ts[2], Ts[3]}, {Ts[4], Ts[5], Ts[6]}};
    integrator.integratePointcloudUndistorted(m, T, &layer, knots);
    if (vgx_scan_stats(integrator.scan(), &counts[0], &counts[1]) != VGX_OK) return 6;
    if (vgx_scan_undistort_stats(integrator.scan(), &counts[2], &counts[3], &counts[4]) != VGX_OK) return 6;
    if (integrator.lastPointcloudSize() != counts[0]) return 6;
    points.resize(3 * (size_t)counts[0]);
    rgba.resize(4 * (size_t)counts[0]);
    if (vgx_scan_download(integrator.scan(), points.data(), rgba.data()) != VGX_OK) return 6;
    blocks = layer.getNumberOfAllocatedBlocks();
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 5;
  }
  vgx_ctx_destroy(ctx);
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 7;
  const int32_t K = (int32_t)knots.knot_time.size();
  fwrite(&K, 4, 1, out);
  fwrite(knots.knot_time.data(), 8, knots.knot_time.size(), out);
  fwrite(knots.knot_T.data(), 4, knots.knot_T.size(), out);
  fwrite(counts, 8, 5, out);
  fwrite(points.data(), 4, points.size(), out);
  fwrite(rgba.data(), 1, rgba.size(), out);
  fwrite(&blocks, 4, 1, out);
  fclose(out);
  printf("SCAN_UNDISTORT_SMOKE_OK\n");
  return 0;
}
