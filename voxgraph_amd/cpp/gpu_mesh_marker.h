// Mesh markers on the GPU: voxblox_ros fillMarkerWithMesh [recalled] over a GpuMesh (vgx_mesh_fill_marker).
//
// voxgraph's three rviz meshes are visualization_msgs/Marker TRIANGLE_LISTs (SubmapVisuals, submap_visuals.cpp:36-87):
// marker.points (three f64 per vertex) and marker.colors (four f32 per vertex, shaded by voxblox's ColorMode), with
// mesh_opacity_ in every alpha.  With the meshes already on the GPU (gpu_mesh.h) the two arrays are made there:
//
//   voxgraph_amd::GpuMesh gpu_mesh(ctx);                                          (kept: their buffers are reused)
//   voxgraph_amd::GpuMeshMarker gpu_marker(ctx);
//   visualization_msgs::Marker marker;
//   marker.header.frame_id = mission_frame;  marker.header.stamp = ros::Time::now();        (the caller's, as publishMesh)
//
//   publishCombinedMesh:   CombinedMeshMarkerOnGpu(submap_collection, &gpu_layer, min_weight, mesh_opacity_, &gpu_mesh, &gpu_marker);
//   publishSeparatedMesh:  SeparatedMeshMarkerOnGpu(submap_collection, min_weight, mesh_opacity_, &gpu_mesh, &gpu_marker);
//   publishMesh:           (gpu_mesh: the active submap's mesh)
//                          ColoredMeshMarkerOnGpu(gpu_mesh, SubmapColor(submap_id), mesh_opacity_, &gpu_marker);
//   then                   DownloadMarker(gpu_marker, &marker);  publisher.publish(marker);
//
// Rules, refusals and what is out of scope are stated at vgx_mesh_fill_marker in include/voxgraph_amd.h.
#ifndef VOXGRAPH_AMD_CPP_GPU_MESH_MARKER_H_
#define VOXGRAPH_AMD_CPP_GPU_MESH_MARKER_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "gpu_mesh.h"

namespace voxgraph_amd {

// voxblox::ColorMode, in its order [recalled]
enum class MarkerColorMode : int32_t {
  kColor = VGX_MARKER_COLOR,
  kHeight = VGX_MARKER_HEIGHT,
  kNormals = VGX_MARKER_NORMALS,
  kGray = VGX_MARKER_GRAY,
  kLambert = VGX_MARKER_LAMBERT,
  kLambertColor = VGX_MARKER_LAMBERT_COLOR
};

constexpr int kMarkerTriangleList = 11;  // visualization_msgs::Marker::TRIANGLE_LIST

// marker.points and marker.colors on the GPU (vgx_mesh_marker): [3T][3] f64 and [3T][4] f32 in soup order.
class GpuMeshMarker {
 public:
  explicit GpuMeshMarker(vgx_ctx ctx) : ctx_(ctx) {
    if (vgx_mesh_marker_create(ctx, &marker_) != VGX_OK)
      throw std::runtime_error(std::string("vgx_mesh_marker_create: ") + vgx_last_error(ctx));
  }
  ~GpuMeshMarker() { vgx_mesh_marker_destroy(marker_); }
  GpuMeshMarker(const GpuMeshMarker&) = delete;
  GpuMeshMarker& operator=(const GpuMeshMarker&) = delete;
  vgx_mesh_marker handle() const { return marker_; }
  const char* last_error() const { return vgx_last_error(ctx_); }
  void stats(int64_t* n_points, int32_t* color_mode) const { check(vgx_mesh_marker_stats(marker_, n_points, color_mode), "vgx_mesh_marker_stats"); }
  // points [n][3] f64, colors [n][4] f32; either may be nullptr
  void download(double* points, float* colors) const { check(vgx_mesh_marker_download(marker_, points, colors), "vgx_mesh_marker_download"); }
  void devicePointers(const double** points, const float** colors) const {
    check(vgx_mesh_marker_device_pointers(marker_, points, colors), "vgx_mesh_marker_device_pointers");
  }
  // the opacity of the last fill (what DownloadMarker writes into marker.color.a)
  float opacity() const { return opacity_; }
  void setOpacity(float opacity) { opacity_ = opacity; }

 private:
  void check(int rc, const char* what) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string(what) + ": " + vgx_last_error(ctx_));
  }
  vgx_ctx ctx_;
  vgx_mesh_marker marker_ = nullptr;
  float opacity_ = 1.0f;
};

// fillMarkerWithMesh with every field of the config
inline GpuMeshMarker& FillMarkerWithMeshOnGpu(const GpuMesh& mesh, const vgx_mesh_marker_config& cfg, GpuMeshMarker* marker) {
  if (!marker) throw std::invalid_argument("FillMarkerWithMeshOnGpu: marker == nullptr");
  if (vgx_mesh_fill_marker(mesh.handle(), &cfg, marker->handle()) != VGX_OK)
    throw std::runtime_error(std::string("vgx_mesh_fill_marker: ") + mesh.last_error());
  marker->setOpacity(cfg.opacity);
  return *marker;
}

// fillMarkerWithMesh(mesh_layer, color_mode, &marker), then SubmapVisuals' opacity in every alpha
inline GpuMeshMarker& FillMarkerWithMeshOnGpu(const GpuMesh& mesh, MarkerColorMode color_mode, float opacity, GpuMeshMarker* marker) {
  vgx_mesh_marker_config cfg;
  vgx_mesh_marker_config_default(&cfg);
  cfg.color_mode = static_cast<int32_t>(color_mode);
  cfg.opacity = opacity;
  return FillMarkerWithMeshOnGpu(mesh, cfg, marker);
}

// SubmapVisuals::publishMesh: cblox colorMeshLayer(color) on one submap's or layer's mesh, then kLambertColor
inline GpuMeshMarker& ColoredMeshMarkerOnGpu(const GpuMesh& mesh, const voxblox::Color& color, float opacity, GpuMeshMarker* marker) {
  vgx_mesh_marker_config cfg;
  vgx_mesh_marker_config_default(&cfg);
  cfg.color_mode = VGX_MARKER_LAMBERT_COLOR;
  cfg.opacity = opacity;
  cfg.use_constant_color = 1;
  cfg.constant_rgba[0] = color.r;
  cfg.constant_rgba[1] = color.g;
  cfg.constant_rgba[2] = color.b;
  cfg.constant_rgba[3] = color.a;
  return FillMarkerWithMeshOnGpu(mesh, cfg, marker);
}

// SubmapVisuals::publishCombinedMesh: the projected map into gpu_layer, its mesh into `mesh`, the marker in kNormals.
// On a mesh with one colour per vertex (gpu_mesh.h, use_color) kColor and kLambertColor shade every vertex with its own
// colour; nothing else in this header depends on the layout.  use_color (off by default) makes such a mesh here, for a
// color_mode that shows it.
template <typename CollectionT>
GpuMeshMarker& CombinedMeshMarkerOnGpu(const CollectionT& collection, GpuTsdfLayer* gpu_layer, float min_weight, float opacity,
                                       GpuMesh* mesh, GpuMeshMarker* marker, bool use_color = false,
                                       MarkerColorMode color_mode = MarkerColorMode::kNormals) {
  GenerateCombinedMeshOnGpu(collection, gpu_layer, min_weight, mesh, use_color);
  return FillMarkerWithMeshOnGpu(*mesh, color_mode, opacity, marker);
}

// SubmapVisuals::publishSeparatedMesh: every submap in voxgraph's colour into `mesh`, the marker in kLambertColor
template <typename CollectionT>
GpuMeshMarker& SeparatedMeshMarkerOnGpu(const CollectionT& collection, float min_weight, float opacity, GpuMesh* mesh,
                                        GpuMeshMarker* marker) {
  GenerateSeparatedMeshOnGpu(collection, min_weight, mesh);
  return FillMarkerWithMeshOnGpu(*mesh, MarkerColorMode::kLambertColor, opacity, marker);
}

// Fills a visualization_msgs::Marker-shaped message: points and colors sized and filled with one copy each, and the
// fixed fields as fillMarkerWithMesh and SubmapVisuals::publishMesh leave them.  The header is the caller's.
template <typename MarkerT>
void DownloadMarker(const GpuMeshMarker& gpu_marker, MarkerT* marker) {
  if (!marker) throw std::invalid_argument("DownloadMarker: marker == nullptr");
  using PointT = typename std::decay<decltype(marker->points[0])>::type;
  using ColorT = typename std::decay<decltype(marker->colors[0])>::type;
  static_assert(sizeof(PointT) == 3 * sizeof(double), "marker.points: three packed f64 (geometry_msgs::Point)");
  static_assert(sizeof(ColorT) == 4 * sizeof(float), "marker.colors: four packed f32 (std_msgs::ColorRGBA)");
  int64_t n = 0;
  gpu_marker.stats(&n, nullptr);
  marker->points.resize(static_cast<size_t>(n));
  marker->colors.resize(static_cast<size_t>(n));
  if (n > 0)
    gpu_marker.download(reinterpret_cast<double*>(marker->points.data()), reinterpret_cast<float*>(marker->colors.data()));
  marker->type = kMarkerTriangleList;
  marker->ns = "mesh";
  marker->scale.x = 1.0;
  marker->scale.y = 1.0;
  marker->scale.z = 1.0;
  marker->pose.orientation.x = 0.0;
  marker->pose.orientation.y = 0.0;
  marker->pose.orientation.z = 0.0;
  marker->pose.orientation.w = 1.0;
  marker->color.a = gpu_marker.opacity();
  marker->frame_locked = true;
}

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_MESH_MARKER_H_
