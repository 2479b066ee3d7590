// Host-side mirror of voxgraph::PointcloudIntegrator
// (voxgraph/src/frontend/measurement_processors/pointcloud_integrator.cpp:23-90): the whole per-frame function, from the
// raw sensor_msgs/PointCloud2 to the integrated layer.
//   field detection                                   :33-43   a field named "rgb" wins, else "intensity", else none
//   pcl::fromROSMsg + voxblox::convertPointcloud      :45-63   -> vgx_scan_decode_msg (the device drops the points that
//                                                              are not finite and makes the colours)
//   new voxblox::FastTsdfIntegrator(config, layer)    :66-71   created at the first message
//   tsdf_integrator_->setLayer(layer)                 :77
//   tsdf_integrator_->integratePointCloud(T, ...)     :83      -> vgx_tsdf_integrate_scan
// No ROS, PCL or voxblox headers are needed: integratePointcloud is templated on the message type and reads the members
// sensor_msgs::PointCloud2 has (fields[d].name / .offset / .datatype / .count, width, height, point_step, row_step,
// is_bigendian, data), so it compiles against the real message and against a stand-in alike.
// Stated deviations: x / y / z must be FLOAT32 with count 1 and an "intensity" field must be FLOAT32 -- PCL's field
// mapping would warn and leave zeros; here the message is refused (std::invalid_argument).  The datatype of "rgb" is
// ignored, which is what the reference's own hack (:38-39) amounts to.
//
// Not in the reference class, which is fed a cloud that lidar_undistortion has corrected already (arche_demo.launch:6,12):
// integratePointcloudUndistorted decodes with vgx_scan_decode_msg_undistorted -- every point moved into the sensor frame
// at the scan's reference time by a pose track (GpuScanTrack), its time taken from the field timeFieldOf finds.
#ifndef VOXGRAPH_AMD_CPP_GPU_POINTCLOUD_INTEGRATOR_H_
#define VOXGRAPH_AMD_CPP_GPU_POINTCLOUD_INTEGRATOR_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_fast_tsdf_integrator.h"
#include "voxgraph_amd.h"

namespace voxgraph_amd {

// Samples (t, T_fixed_sensor) of the sensor's pose in any fixed frame (odometry), and the vgx_scan_track they make for
// one scan: knot k holds T_ref^-1 * T_k, the sensor at t_k in the sensor frame at the scan's reference time, and
// t_k - stamp, the time since the message's stamp.  All of it in f64, one rounding per operation (capi.ScanTrack does the
// same arithmetic and gives the same bytes):
//   r      the reference's inverse rotation: n = sqrt(((w w + x x) + y y) + z z) of q_ref, r = (w / n, -x / n, -y / n, -z / n)
//   q_rel  r (x) q_k, Hamilton product, every component summed left to right:
//          w = rw kw - rx kx - ry ky - rz kz        x = rw kx + rx kw + ry kz - rz ky
//          y = rw ky - rx kz + ry kw + rz kx        z = rw kz + rx ky - ry kx + rz kw
//          then divided by m = sqrt(((w w + x x) + y y) + z z)
//   t_rel  r applied to d = t_k - t_ref as the library applies a transform: uv = r.v x d, uv += uv, cc = r.v x uv,
//          t_rel = (d + rw uv) + cc
//   knot_time[k] = t_k - stamp; knot_T[k] = (q_rel, t_rel) cast to f32.
class GpuScanTrack {
 public:
  // what relativeTo returns: the arrays a vgx_scan_track points into, and the stamp the knot times are relative to
  struct Knots {
    std::vector<double> knot_time;
    std::vector<float> knot_T;  // [n][7]
    double stamp_seconds = 0.0;
    vgx_scan_track view() const { return vgx_scan_track{(int32_t)knot_time.size(), knot_time.data(), knot_T.data()}; }
  };

  // T_fixed_sensor: {qw,qx,qy,qz, tx,ty,tz}; times strictly ascending (the decode refuses a track whose are not)
  void add7(double t, const double T_fixed_sensor[7]) {
    times_.push_back(t);
    poses_.insert(poses_.end(), T_fixed_sensor, T_fixed_sensor + 7);
  }
  // the same from a kindr::minimal transformation (QuatTransformationTemplate<double> keeps every bit)
  template <class Transformation>
  void add(double t, const Transformation& T_fixed_sensor) {
    const auto& q = T_fixed_sensor.getRotation();
    const auto& p = T_fixed_sensor.getPosition();
    const double T[7] = {(double)q.w(), (double)q.x(), (double)q.y(), (double)q.z(), (double)p[0], (double)p[1], (double)p[2]};
    add7(t, T);
  }
  size_t size() const { return times_.size(); }
  void clear() {
    times_.clear();
    poses_.clear();
  }

  // The track for a scan whose reference frame is the sensor at T_fixed_sensor_ref and whose stamp is stamp_seconds.
  template <class Transformation>
  Knots relativeTo(const Transformation& T_fixed_sensor_ref, double stamp_seconds = 0.0) const {
    const auto& q = T_fixed_sensor_ref.getRotation();
    const auto& p = T_fixed_sensor_ref.getPosition();
    const double T[7] = {(double)q.w(), (double)q.x(), (double)q.y(), (double)q.z(), (double)p[0], (double)p[1], (double)p[2]};
    return relativeTo7(T, stamp_seconds);
  }
  // the same with the reference as {qw,qx,qy,qz, tx,ty,tz}
  Knots relativeTo7(const double T_fixed_sensor_ref[7], double stamp_seconds = 0.0) const {
    Knots out;
    out.stamp_seconds = stamp_seconds;
    const double* ref = T_fixed_sensor_ref;
    const double n = std::sqrt(((ref[0] * ref[0] + ref[1] * ref[1]) + ref[2] * ref[2]) + ref[3] * ref[3]);
    const double rw = ref[0] / n, rx = -ref[1] / n, ry = -ref[2] / n, rz = -ref[3] / n;
    for (size_t k = 0; k < times_.size(); ++k) {
      const double* P = &poses_[7 * k];
      const double kw = P[0], kx = P[1], ky = P[2], kz = P[3];
      const double qw = rw * kw - rx * kx - ry * ky - rz * kz;
      const double qx = rw * kx + rx * kw + ry * kz - rz * ky;
      const double qy = rw * ky - rx * kz + ry * kw + rz * kx;
      const double qz = rw * kz + rx * ky - ry * kx + rz * kw;
      const double m = std::sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
      const double dx = P[4] - ref[4], dy = P[5] - ref[5], dz = P[6] - ref[6];
      double ux = ry * dz - rz * dy, uy = rz * dx - rx * dz, uz = rx * dy - ry * dx;
      ux += ux;
      uy += uy;
      uz += uz;
      const double cx = ry * uz - rz * uy, cy = rz * ux - rx * uz, cz = rx * uy - ry * ux;
      const double T[7] = {qw / m, qx / m, qy / m, qz / m, (dx + rw * ux) + cx, (dy + rw * uy) + cy, (dz + rw * uz) + cz};
      out.knot_time.push_back(times_[k] - stamp_seconds);
      for (int j = 0; j < 7; ++j) out.knot_T.push_back((float)T[j]);
    }
    return out;
  }

 private:
  std::vector<double> times_, poses_;
};

class GpuPointcloudIntegrator {
 public:
  static constexpr uint8_t kUint32 = 6;   // sensor_msgs::PointField::UINT32
  static constexpr uint8_t kFloat32 = 7;  // sensor_msgs::PointField::FLOAT32
  static constexpr uint8_t kFloat64 = 8;  // sensor_msgs::PointField::FLOAT64

  explicit GpuPointcloudIntegrator(vgx_ctx ctx) : ctx_(ctx) {
    vgx_tsdf_config_default(&tsdf_integrator_config_);
    vgx_scan_config_default(&scan_config_);  // GrayscaleColorMap, setMaxValue(10000.0) (:12-14)
    if (vgx_scan_create(ctx, &scan_) != VGX_OK) throw std::runtime_error(std::string("vgx_scan_create: ") + vgx_last_error(ctx));
  }
  ~GpuPointcloudIntegrator() {
    tsdf_integrator_.reset();
    if (range_image_) vgx_range_image_destroy(range_image_);
    vgx_scan_destroy(scan_);
  }
  GpuPointcloudIntegrator(const GpuPointcloudIntegrator&) = delete;
  GpuPointcloudIntegrator& operator=(const GpuPointcloudIntegrator&) = delete;

  // setTsdfIntegratorConfigFromRosParam (:17-21) with the config already read; takes effect when the integrator is made
  void setTsdfIntegratorConfig(const GpuFastTsdfIntegrator::Config& config) { tsdf_integrator_config_ = config; }
  void setScanConfig(const vgx_scan_config& config) { scan_config_ = config; }

  // The layout of a message: the reference's field detection, and the refusals stated at the top.
  template <class Msg>
  static vgx_scan_layout layoutOf(const Msg& msg) {
    vgx_scan_layout l{};
    l.width = msg.width;
    l.height = msg.height;
    l.point_step = msg.point_step;
    l.row_step = msg.row_step;
    l.is_bigendian = msg.is_bigendian ? 1 : 0;
    l.color_kind = VGX_SCAN_COLOR_NONE;
    bool color_pointcloud = false, has_intensity = false, has[3] = {false, false, false};
    uint32_t intensity_offset = 0;
    for (size_t d = 0; d < msg.fields.size(); ++d) {
      const auto& f = msg.fields[d];
      const std::string name = f.name;
      if (name == "rgb") {
        color_pointcloud = true;
        l.color_offset = f.offset;
      } else if (name == "intensity") {
        if (f.datatype != kFloat32) throw std::invalid_argument("integratePointcloud: the intensity field is not FLOAT32");
        has_intensity = true;
        intensity_offset = f.offset;
      } else if (name == "x" || name == "y" || name == "z") {
        if (f.datatype != kFloat32 || f.count != 1)
          throw std::invalid_argument("integratePointcloud: field " + name + " is not one FLOAT32");
        const int k = name[0] - 'x';
        has[k] = true;
        (k == 0 ? l.offset_x : (k == 1 ? l.offset_y : l.offset_z)) = f.offset;
      }
    }
    if (!has[0] || !has[1] || !has[2]) throw std::invalid_argument("integratePointcloud: the message has no x, y or z field");
    if (color_pointcloud) {
      l.color_kind = VGX_SCAN_COLOR_RGB;
    } else if (has_intensity) {
      l.color_kind = VGX_SCAN_COLOR_INTENSITY;
      l.color_offset = intensity_offset;
    }
    return l;
  }

  // The per-point time of a message in seconds since its stamp: the first of these fields, each with count 1 (driver
  // conventions, defined here; the checks run in this order whatever the order of msg.fields)
  //   "t"          UINT32   nanoseconds since the stamp (Ouster)                 scale 1e-9, offset 0
  //   "time"       FLOAT32  seconds since the stamp (Velodyne)                   scale 1,    offset 0
  //   "timestamp"  FLOAT64  absolute seconds                                     scale 1,    offset -stamp_seconds
  // anything else: std::invalid_argument.
  template <class Msg>
  static vgx_scan_time_field timeFieldOf(const Msg& msg, double stamp_seconds) {
    struct Rule {
      const char* name;
      uint8_t datatype;
      int32_t kind;
      double scale, offset_s;
    };
    const Rule rules[3] = {{"t", kUint32, VGX_SCAN_TIME_UINT32, 1e-9, 0.0},
                           {"time", kFloat32, VGX_SCAN_TIME_FLOAT32, 1.0, 0.0},
                           {"timestamp", kFloat64, VGX_SCAN_TIME_FLOAT64, 1.0, -stamp_seconds}};
    for (const Rule& r : rules)
      for (size_t d = 0; d < msg.fields.size(); ++d) {
        const auto& f = msg.fields[d];
        if (std::string(f.name) == r.name && f.datatype == r.datatype && f.count == 1)
          return vgx_scan_time_field{r.kind, (uint32_t)f.offset, r.scale, r.offset_s};
      }
    throw std::invalid_argument("integratePointcloudUndistorted: the message has no t (UINT32), time (FLOAT32) or timestamp (FLOAT64) field");
  }

  // integratePointcloud(pointcloud_msg, T_submap_sensor, submap_ptr) with the submap's TSDF layer
  //   Transformation  kindr::minimal::QuatTransformationTemplate<float>: getRotation().{w,x,y,z}(), getPosition()[k]
  // Returns with the scan queued (voxblox's void call).
  template <class Msg, class Transformation>
  void integratePointcloud(const Msg& msg, const Transformation& T_submap_sensor, GpuTsdfLayer* layer) {
    const auto& q = T_submap_sensor.getRotation();
    const auto& t = T_submap_sensor.getPosition();
    const float T[7] = {(float)q.w(), (float)q.x(), (float)q.y(), (float)q.z(), (float)t[0], (float)t[1], (float)t[2]};
    integratePointcloud7(msg, T, layer);
  }
  // the same with the transform as {qw,qx,qy,qz, tx,ty,tz}
  template <class Msg>
  void integratePointcloud7(const Msg& msg, const float T_submap_sensor[7], GpuTsdfLayer* layer) {
    integrate7(msg, T_submap_sensor, layer, nullptr);
  }

  // The same for a sweep taken while the sensor moved: every point is first moved into the sensor frame at the scan's
  // reference time -- the frame T_submap_sensor_ref places in the submap -- by `track` (GpuScanTrack::relativeTo of the
  // sensor's pose at that reference time, with the message's stamp in seconds).
  template <class Msg, class Transformation>
  void integratePointcloudUndistorted(const Msg& msg, const Transformation& T_submap_sensor_ref, GpuTsdfLayer* layer,
                                      const GpuScanTrack::Knots& track) {
    const auto& q = T_submap_sensor_ref.getRotation();
    const auto& t = T_submap_sensor_ref.getPosition();
    const float T[7] = {(float)q.w(), (float)q.x(), (float)q.y(), (float)q.z(), (float)t[0], (float)t[1], (float)t[2]};
    integrate7(msg, T, layer, &track);
  }

  // The projective route for a spinning LiDAR (include/voxgraph_amd.h, "LiDAR range images"): the message decoded as
  // above, its points gathered into the range image of `model` (the nearest return per pixel), and every voxel near a
  // return updated from the ONE pixel it projects into -- no rays, the same layer bit for bit on every run.  Returns with
  // the frame queued unless `counts` is given.  The integrator's configuration and layer are integratePointcloud's.
  template <class Msg, class Transformation>
  void integrateProjective(const Transformation& T_submap_sensor, const Msg& msg, const vgx_lidar_model& model, GpuTsdfLayer* layer,
                           vgx_projective_counts* counts = nullptr) {
    if (vgx_range_image_check(&model) != VGX_OK) throw std::invalid_argument("integrateProjective: the LiDAR model is refused");
    integrateProjectiveBy(T_submap_sensor, msg, layer, counts, "vgx_range_image_build",
                          [&](vgx_range_image image, vgx_scan scan) { return vgx_range_image_build(image, &model, scan, nullptr); });
  }
  // The same for a sensor described by a beam table (include/voxgraph_amd.h, "LiDAR range images: beam tables"): rows with
  // elevations and azimuth offsets of their own, strictly monotone -- sortedBeamTable brings a table in laser order there.
  template <class Msg, class Transformation>
  void integrateProjective(const Transformation& T_submap_sensor, const Msg& msg, const vgx_lidar_beam_model& model, GpuTsdfLayer* layer,
                           vgx_projective_counts* counts = nullptr) {
    if (vgx_range_image_check_beams(&model) != VGX_OK) throw std::invalid_argument("integrateProjective: the beam table is refused");
    integrateProjectiveBy(T_submap_sensor, msg, layer, counts, "vgx_range_image_build_beams",
                          [&](vgx_range_image image, vgx_scan scan) { return vgx_range_image_build_beams(image, &model, scan, nullptr); });
  }
  // A beam table as sensors publish it -- in laser (firing) order, not monotone -- sorted by ascending elevation, with the
  // permutation: row k of the sorted table is laser order[k].  view() is valid while the object lives and is not changed.
  struct SortedBeamTable {
    std::vector<float> row_elevation_rad, row_azimuth_offset_rad;
    std::vector<int32_t> order;
    vgx_lidar_beam_model view(int32_t width, float azimuth_first_rad, int32_t azimuth_clockwise, float row_half_extent_max_rad) const {
      return vgx_lidar_beam_model{width, (int32_t)row_elevation_rad.size(), azimuth_first_rad, azimuth_clockwise, row_elevation_rad.data(),
                                  row_azimuth_offset_rad.empty() ? nullptr : row_azimuth_offset_rad.data(), row_half_extent_max_rad};
    }
  };
  // azimuth_offset_rad may be NULL (no offsets).  Equal elevations stay in laser order (and the check then refuses the table).
  static SortedBeamTable sortedBeamTable(const float* elevation_rad, const float* azimuth_offset_rad, int32_t n) {
    SortedBeamTable t;
    for (int32_t k = 0; k < n; ++k) t.order.push_back(k);
    std::stable_sort(t.order.begin(), t.order.end(), [&](int32_t a, int32_t b) { return elevation_rad[a] < elevation_rad[b]; });
    for (int32_t k : t.order) {
      t.row_elevation_rad.push_back(elevation_rad[k]);
      if (azimuth_offset_rad) t.row_azimuth_offset_rad.push_back(azimuth_offset_rad[k]);
    }
    return t;
  }
  // the range image of the last integrateProjective (NULL before the first)
  vgx_range_image rangeImage() const { return range_image_; }

  // points of the last message that were integrated ("Integrating a pointcloud with %lu points", :80-81)
  int64_t lastPointcloudSize() const { return last_points_; }
  // the width the integrator was given for the last message: the message's, or 0 (unorganised) when points were dropped
  int32_t lastCloudWidth() const { return last_cloud_width_; }
  vgx_scan scan() const { return scan_; }

 private:
  // build: int(vgx_range_image, vgx_scan), the image of the decoded scan; `what` names it in the error
  template <class Msg, class Transformation, class Build>
  void integrateProjectiveBy(const Transformation& T_submap_sensor, const Msg& msg, GpuTsdfLayer* layer, vgx_projective_counts* counts,
                             const char* what, Build build) {
    const auto& q = T_submap_sensor.getRotation();
    const auto& t = T_submap_sensor.getPosition();
    const float T[7] = {(float)q.w(), (float)q.x(), (float)q.y(), (float)q.z(), (float)t[0], (float)t[1], (float)t[2]};
    if (!layer) throw std::invalid_argument("integrateProjective: NULL layer");
    const vgx_scan_layout layout = layoutOf(msg);
    if (vgx_scan_decode_msg(scan_, &layout, &scan_config_, msg.data.data(), (int64_t)msg.data.size()) != VGX_OK)
      throw std::runtime_error(std::string("vgx_scan_decode_msg: ") + vgx_last_error(ctx_));
    int64_t dropped = 0;
    vgx_scan_stats(scan_, &last_points_, &dropped);
    if (!range_image_ && vgx_range_image_create(ctx_, &range_image_) != VGX_OK)
      throw std::runtime_error(std::string("vgx_range_image_create: ") + vgx_last_error(ctx_));
    if (build(range_image_, scan_) != VGX_OK) throw std::runtime_error(std::string(what) + ": " + vgx_last_error(ctx_));
    if (!tsdf_integrator_) tsdf_integrator_.reset(new GpuFastTsdfIntegrator(ctx_, tsdf_integrator_config_, layer));
    tsdf_integrator_->setLayer(layer);
    if (vgx_tsdf_integrate_range_image(tsdf_integrator_->handle(), T, range_image_, counts) != VGX_OK)
      throw std::runtime_error(std::string("vgx_tsdf_integrate_range_image: ") + vgx_last_error(ctx_));
  }

  template <class Msg>
  void integrate7(const Msg& msg, const float T_submap_sensor[7], GpuTsdfLayer* layer, const GpuScanTrack::Knots* track) {
    if (!layer) throw std::invalid_argument("integratePointcloud: NULL layer");  // CHECK_NOTNULL(submap_ptr)
    const vgx_scan_layout layout = layoutOf(msg);
    if (track) {
      const vgx_scan_time_field field = timeFieldOf(msg, track->stamp_seconds);
      const vgx_scan_track view = track->view();
      if (vgx_scan_decode_msg_undistorted(scan_, &layout, &scan_config_, &field, &view, msg.data.data(), (int64_t)msg.data.size()) !=
          VGX_OK)
        throw std::runtime_error(std::string("vgx_scan_decode_msg_undistorted: ") + vgx_last_error(ctx_));
    } else if (vgx_scan_decode_msg(scan_, &layout, &scan_config_, msg.data.data(), (int64_t)msg.data.size()) != VGX_OK) {
      throw std::runtime_error(std::string("vgx_scan_decode_msg: ") + vgx_last_error(ctx_));
    }
    if (!tsdf_integrator_) tsdf_integrator_.reset(new GpuFastTsdfIntegrator(ctx_, tsdf_integrator_config_, layer));
    tsdf_integrator_->setLayer(layer);
    int64_t dropped = 0;
    vgx_scan_stats(scan_, &last_points_, &dropped);
    // the message's rows survive only when no point was dropped: a compacted cloud is no longer organised
    last_cloud_width_ = dropped == 0 && msg.width <= 0x7fffffffu ? (int32_t)msg.width : 0;
    tsdf_integrator_->setCloudWidth(last_cloud_width_);
    if (vgx_tsdf_integrate_scan(tsdf_integrator_->handle(), T_submap_sensor, scan_, 0, nullptr) != VGX_OK)
      throw std::runtime_error(std::string("vgx_tsdf_integrate_scan: ") + vgx_last_error(ctx_));
  }

  vgx_ctx ctx_;
  GpuFastTsdfIntegrator::Config tsdf_integrator_config_;
  vgx_scan_config scan_config_;
  vgx_scan scan_ = nullptr;
  vgx_range_image range_image_ = nullptr;
  std::unique_ptr<GpuFastTsdfIntegrator> tsdf_integrator_;
  int64_t last_points_ = 0;
  int32_t last_cloud_width_ = 0;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_POINTCLOUD_INTEGRATOR_H_
