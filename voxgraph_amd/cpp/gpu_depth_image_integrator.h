// A depth camera's per-frame function: from the raw sensor_msgs/Image depth frame, its sensor_msgs/CameraInfo and
// (optionally) the registered colour image to the integrated layer.  Not in the reference, whose PointcloudIntegrator is
// fed a cloud (pointcloud_integrator.cpp:23-90): this is what a depth_image_proc nodelet in front of it would do, moved
// into the decode (include/voxgraph_amd.h, "Depth-image scans").
//   image.encoding -> VGX_DEPTH_* / VGX_IMAGE_COLOR_*     depthEncodingOf, colorKindOf
//   image.step, .is_bigendian, .width, .height            layoutOf
//   CameraInfo::K[0], K[4], K[2], K[5]                    cameraOf (on top of camera(): depth unit, gate, strides)
//   decode                                                -> vgx_scan_decode_depth_image[_undistorted]
//   integrateDepthImage                                   decode, then vgx_tsdf_integrate_scan as GpuPointcloudIntegrator does
//   integrateProjective                                   -> vgx_tsdf_integrate_depth_image: per-voxel projective update, no cloud
// No ROS headers are needed: everything is templated on the message types and reads the members sensor_msgs::Image
// (height, width, encoding, is_bigendian, step, data) and sensor_msgs::CameraInfo (K) have, so it compiles against the
// real messages and against stand-ins alike.
// Refused (std::invalid_argument): a depth encoding other than "16UC1", "mono16", "32FC1"; a colour encoding other than
// "rgb8", "bgr8", "rgba8", "bgra8", "mono8"; a colour image whose width or height differs from the depth image's.  The
// image must be rectified (lens distortion is not modelled) and the colour image registered to the depth image.
#ifndef VOXGRAPH_AMD_CPP_GPU_DEPTH_IMAGE_INTEGRATOR_H_
#define VOXGRAPH_AMD_CPP_GPU_DEPTH_IMAGE_INTEGRATOR_H_

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>

#include "gpu_fast_tsdf_integrator.h"
#include "gpu_pointcloud_integrator.h"
#include "voxgraph_amd.h"

namespace voxgraph_amd {

class GpuDepthImageIntegrator {
 public:
  explicit GpuDepthImageIntegrator(vgx_ctx ctx) : ctx_(ctx) {
    vgx_tsdf_config_default(&tsdf_integrator_config_);
    vgx_scan_config_default(&scan_config_);
    vgx_depth_camera_default(&camera_);
    if (vgx_scan_create(ctx, &scan_) != VGX_OK) throw std::runtime_error(std::string("vgx_scan_create: ") + vgx_last_error(ctx));
  }
  ~GpuDepthImageIntegrator() {
    tsdf_integrator_.reset();
    vgx_scan_destroy(scan_);
  }
  GpuDepthImageIntegrator(const GpuDepthImageIntegrator&) = delete;
  GpuDepthImageIntegrator& operator=(const GpuDepthImageIntegrator&) = delete;

  // takes effect when the integrator is made, at the first frame
  void setTsdfIntegratorConfig(const GpuFastTsdfIntegrator::Config& config) { tsdf_integrator_config_ = config; }
  void setScanConfig(const vgx_scan_config& config) { scan_config_ = config; }  // constant_rgba: the colour without a colour image
  // depth_unit_m, the depth gate and the strides of the frames to come (fx, fy, cx, cy are taken from every frame's CameraInfo)
  vgx_depth_camera& camera() { return camera_; }

  template <class Image>
  static int32_t depthEncodingOf(const Image& depth) {
    const std::string e = depth.encoding;
    if (e == "16UC1" || e == "mono16") return VGX_DEPTH_16UC1;
    if (e == "32FC1") return VGX_DEPTH_32FC1;
    throw std::invalid_argument("integrateDepthImage: the depth encoding " + e + " is not 16UC1, mono16 or 32FC1");
  }
  template <class Image>
  static int32_t colorKindOf(const Image& color) {
    const std::string e = color.encoding;
    if (e == "rgb8") return VGX_IMAGE_COLOR_RGB8;
    if (e == "bgr8") return VGX_IMAGE_COLOR_BGR8;
    if (e == "rgba8") return VGX_IMAGE_COLOR_RGBA8;
    if (e == "bgra8") return VGX_IMAGE_COLOR_BGRA8;
    if (e == "mono8") return VGX_IMAGE_COLOR_MONO8;
    throw std::invalid_argument("integrateDepthImage: the colour encoding " + e + " is not rgb8, bgr8, rgba8, bgra8 or mono8");
  }
  // the layout of a depth image and (color != nullptr) its registered colour image
  template <class Image>
  static vgx_depth_image_layout layoutOf(const Image& depth, const Image* color) {
    vgx_depth_image_layout l{};
    l.width = depth.width;
    l.height = depth.height;
    l.row_step = depth.step;
    l.encoding = depthEncodingOf(depth);
    l.is_bigendian = depth.is_bigendian ? 1 : 0;
    l.color_kind = VGX_IMAGE_COLOR_NONE;
    if (color) {
      if (color->width != depth.width || color->height != depth.height)
        throw std::invalid_argument("integrateDepthImage: the colour image's size differs from the depth image's");
      l.color_kind = colorKindOf(*color);
      l.color_row_step = color->step;
    }
    return l;
  }
  // camera() with the pinhole model of a CameraInfo: K is row-major [fx 0 cx; 0 fy cy; 0 0 1]
  template <class CameraInfo>
  vgx_depth_camera cameraOf(const CameraInfo& info) const {
    return cameraFrom(camera_, info);
  }
  template <class CameraInfo>
  static vgx_depth_camera cameraFrom(const vgx_depth_camera& base, const CameraInfo& info) {
    vgx_depth_camera c = base;
    c.fx = info.K[0];
    c.fy = info.K[4];
    c.cx = info.K[2];
    c.cy = info.K[5];
    return c;
  }

  // decode alone: afterwards scan() holds the frame's points in the optical frame, as after vgx_scan_decode_msg
  template <class Image, class CameraInfo>
  void decode(const Image& depth, const CameraInfo& info, const Image* color) {
    decodeWith(depth, info, color, nullptr, nullptr);
  }
  // the same for a rolling-shutter frame taken while the camera moved: row v was exposed at row_time.offset_s + v *
  // row_time.scale seconds after the stamp the track's knot times are relative to (GpuScanTrack::relativeTo)
  template <class Image, class CameraInfo>
  void decodeUndistorted(const Image& depth, const CameraInfo& info, const Image* color, const vgx_depth_row_time& row_time,
                         const GpuScanTrack::Knots& track) {
    decodeWith(depth, info, color, &row_time, &track);
  }

  // The frame integrated into the submap's TSDF layer with the camera's optical frame at T_submap_camera.
  //   Transformation  kindr::minimal::QuatTransformationTemplate<float>: getRotation().{w,x,y,z}(), getPosition()[k]
  // Returns with the scan queued (voxblox's void call).
  template <class Transformation, class Image, class CameraInfo>
  void integrateDepthImage(const Transformation& T_submap_camera, const Image& depth, const CameraInfo& info, const Image* color,
                           GpuTsdfLayer* layer) {
    if (!layer) throw std::invalid_argument("integrateDepthImage: NULL layer");
    decode(depth, info, color);
    integrateScan(T_submap_camera, layer);
  }
  template <class Transformation, class Image, class CameraInfo>
  void integrateDepthImageUndistorted(const Transformation& T_submap_camera_ref, const Image& depth, const CameraInfo& info,
                                      const Image* color, GpuTsdfLayer* layer, const vgx_depth_row_time& row_time,
                                      const GpuScanTrack::Knots& track) {
    if (!layer) throw std::invalid_argument("integrateDepthImage: NULL layer");
    decodeUndistorted(depth, info, color, row_time, track);
    integrateScan(T_submap_camera_ref, layer);
  }

  // The frame integrated PROJECTIVELY (include/voxgraph_amd.h, "Projective depth-image integration"): every voxel in view
  // looks up its pixel; no cloud is decoded, scan() and lastPointcloudSize() keep what they held.  The strides of camera()
  // are not read, the scan config is not used (a frame without a colour image is integrated opaque white).  counts ==
  // nullptr: returns with the frame queued (voxblox's void call); else the frame's counts, and the call waits for it.
  template <class Transformation, class Image, class CameraInfo>
  void integrateProjective(const Transformation& T_submap_camera, const Image& depth, const CameraInfo& info, const Image* color,
                           GpuTsdfLayer* layer, vgx_projective_counts* counts = nullptr) {
    if (!layer) throw std::invalid_argument("integrateProjective: NULL layer");
    const vgx_depth_image_layout layout = layoutOf(depth, color);
    const vgx_depth_camera cam = cameraOf(info);
    const auto& q = T_submap_camera.getRotation();
    const auto& t = T_submap_camera.getPosition();
    const float T[7] = {(float)q.w(), (float)q.x(), (float)q.y(), (float)q.z(), (float)t[0], (float)t[1], (float)t[2]};
    if (!tsdf_integrator_) tsdf_integrator_.reset(new GpuFastTsdfIntegrator(ctx_, tsdf_integrator_config_, layer));
    tsdf_integrator_->setLayer(layer);
    if (vgx_tsdf_integrate_depth_image(tsdf_integrator_->handle(), T, &layout, &cam, depth.data.data(), (int64_t)depth.data.size(),
                                       color ? color->data.data() : nullptr, color ? (int64_t)color->data.size() : 0,
                                       counts) != VGX_OK)
      throw std::runtime_error(std::string("vgx_tsdf_integrate_depth_image: ") + vgx_last_error(ctx_));
  }
  template <class Transformation, class Image, class CameraInfo>
  void integrateProjective(const Transformation& T_submap_camera, const Image& depth, const CameraInfo& info, GpuTsdfLayer* layer) {
    integrateProjective(T_submap_camera, depth, info, static_cast<const Image*>(nullptr), layer);
  }

  // points of the last frame that were kept
  int64_t lastPointcloudSize() const { return last_points_; }
  vgx_scan scan() const { return scan_; }

 private:
  template <class Image, class CameraInfo>
  void decodeWith(const Image& depth, const CameraInfo& info, const Image* color, const vgx_depth_row_time* row_time,
                  const GpuScanTrack::Knots* track) {
    const vgx_depth_image_layout layout = layoutOf(depth, color);
    const vgx_depth_camera cam = cameraOf(info);
    const void* color_data = color ? color->data.data() : nullptr;
    const int64_t color_bytes = color ? (int64_t)color->data.size() : 0;
    if (track) {
      const vgx_scan_track view = track->view();
      if (vgx_scan_decode_depth_image_undistorted(scan_, &layout, &cam, &scan_config_, row_time, &view, depth.data.data(),
                                                  (int64_t)depth.data.size(), color_data, color_bytes) != VGX_OK)
        throw std::runtime_error(std::string("vgx_scan_decode_depth_image_undistorted: ") + vgx_last_error(ctx_));
    } else if (vgx_scan_decode_depth_image(scan_, &layout, &cam, &scan_config_, depth.data.data(), (int64_t)depth.data.size(),
                                           color_data, color_bytes) != VGX_OK) {
      throw std::runtime_error(std::string("vgx_scan_decode_depth_image: ") + vgx_last_error(ctx_));
    }
    vgx_scan_stats(scan_, &last_points_, nullptr);
  }

  template <class Transformation>
  void integrateScan(const Transformation& T_submap_camera, GpuTsdfLayer* layer) {
    const auto& q = T_submap_camera.getRotation();
    const auto& t = T_submap_camera.getPosition();
    const float T[7] = {(float)q.w(), (float)q.x(), (float)q.y(), (float)q.z(), (float)t[0], (float)t[1], (float)t[2]};
    if (!tsdf_integrator_) tsdf_integrator_.reset(new GpuFastTsdfIntegrator(ctx_, tsdf_integrator_config_, layer));
    tsdf_integrator_->setLayer(layer);
    tsdf_integrator_->setCloudWidth(0);  // a compacted frame is no longer organised
    if (vgx_tsdf_integrate_scan(tsdf_integrator_->handle(), T, scan_, 0, nullptr) != VGX_OK)
      throw std::runtime_error(std::string("vgx_tsdf_integrate_scan: ") + vgx_last_error(ctx_));
  }

  vgx_ctx ctx_;
  GpuFastTsdfIntegrator::Config tsdf_integrator_config_;
  vgx_scan_config scan_config_;
  vgx_depth_camera camera_;
  vgx_scan scan_ = nullptr;
  std::unique_ptr<GpuFastTsdfIntegrator> tsdf_integrator_;
  int64_t last_points_ = 0;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_DEPTH_IMAGE_INTEGRATOR_H_
