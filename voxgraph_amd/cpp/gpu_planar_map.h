// The planar map for a 2D planner: a layer's height band as a nav_msgs/OccupancyGrid and a planar distance field.
//
// The robots voxgraph was flown and walked on steer through an OccupancyGrid or a 2D distance slice.  GpuPlanarMap fills
// both from a device layer -- a vgx_tsdf_layer (the active submap, the projected map) or a finished vgx_submap's raw TSDF
// or ESDF layer -- in one call; the collapse along z and the distance transform run on the device (vgx_planar.hip), and
// what crosses to the host is the grid.  Rules (band, voxel classes, state, box, distance): include/voxgraph_amd.h,
// "Planar map".
//
// ROS is not a dependency: the message type is a template parameter, and anything with nav_msgs/OccupancyGrid's fields
// -- info.resolution, info.width, info.height, info.origin.position.{x, y, z}, data (std::vector<int8_t>) -- will do
// (tests/cpp/occupancy_grid_standin.h is the one the tests use).  The header and info.map_load_time are the caller's.
#ifndef VOXGRAPH_AMD_CPP_GPU_PLANAR_MAP_H_
#define VOXGRAPH_AMD_CPP_GPU_PLANAR_MAP_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "voxgraph_amd.h"

namespace voxgraph_amd {

// vgx_planar_map_config_default() with the band set: there is no default band
inline vgx_planar_map_config PlanarMapConfig(float z_min, float z_max) {
  vgx_planar_map_config cfg;
  vgx_planar_map_config_default(&cfg);
  cfg.z_min = z_min;
  cfg.z_max = z_max;
  return cfg;
}

// A vgx_planar_map owned for the length of a scope (reuse one across calls: its device buffers grow on demand).
class GpuPlanarMap {
 public:
  explicit GpuPlanarMap(vgx_ctx ctx) : ctx_(ctx) {
    if (vgx_planar_map_create(ctx, &h_) != VGX_OK) throw std::runtime_error(std::string("vgx_planar_map_create: ") + vgx_last_error(ctx));
  }
  GpuPlanarMap(const GpuPlanarMap&) = delete;
  GpuPlanarMap& operator=(const GpuPlanarMap&) = delete;
  ~GpuPlanarMap() {
    if (h_) vgx_planar_map_destroy(h_);
  }
  vgx_planar_map handle() const { return h_; }

  // the producing calls: the map is complete when they return
  void update(vgx_tsdf_layer layer, const vgx_planar_map_config& cfg) { check(vgx_tsdf_layer_planar_map(layer, &cfg, h_)); }
  void update(vgx_submap submap, int32_t layer, const vgx_planar_map_config& cfg) {
    check(vgx_submap_layer_planar_map(submap, layer, &cfg, h_));
  }

  int32_t width() const { return dim(0); }
  int32_t height() const { return dim(1); }
  // cells in state 0 (unknown), 1 (free), 2 (occupied)
  void counts(int64_t out[3]) const { check(vgx_planar_map_stats(h_, nullptr, nullptr, nullptr, out)); }

  // The grid as an OccupancyGrid: data -1 / 0 / 100, row-major from the origin corner, x fastest; `z` is the height the
  // caller wants the grid drawn at (the band's middle, say).
  template <class OccupancyGridT>
  void toOccupancyGrid(OccupancyGridT* msg, double z = 0.0) const {
    int32_t mn[2], dm[2];
    float vs = 0.0f;
    check(vgx_planar_map_stats(h_, mn, dm, &vs, nullptr));
    msg->info.resolution = vs;
    msg->info.width = static_cast<uint32_t>(dm[0]);
    msg->info.height = static_cast<uint32_t>(dm[1]);
    msg->info.origin.position.x = static_cast<double>(static_cast<float>(mn[0]) * vs);
    msg->info.origin.position.y = static_cast<double>(static_cast<float>(mn[1]) * vs);
    msg->info.origin.position.z = z;
    msg->data.resize(static_cast<size_t>(dm[0]) * static_cast<size_t>(dm[1]));
    check(vgx_planar_map_download(h_, nullptr, msg->data.data(), nullptr, nullptr, nullptr));
  }
  // the planar distance to the nearest obstacle cell (metres, clipped to max_distance_m), the same cell order
  std::vector<float> distanceField() const {
    std::vector<float> out(cells());
    check(vgx_planar_map_download(h_, nullptr, nullptr, nullptr, nullptr, out.data()));
    return out;
  }
  // the smallest distance of each cell's column, and the height of its highest occupied voxel
  void columns(std::vector<float>* clearance, std::vector<float>* obstacle_height) const {
    clearance->resize(cells());
    obstacle_height->resize(cells());
    check(vgx_planar_map_download(h_, nullptr, nullptr, clearance->data(), obstacle_height->data(), nullptr));
  }

 private:
  int32_t dim(int a) const {
    int32_t dm[2] = {0, 0};
    check(vgx_planar_map_stats(h_, nullptr, dm, nullptr, nullptr));
    return dm[a];
  }
  size_t cells() const { return static_cast<size_t>(width()) * static_cast<size_t>(height()); }
  void check(int rc) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string("planar map: ") + vgx_last_error(ctx_));
  }
  vgx_ctx ctx_;
  vgx_planar_map h_ = nullptr;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_PLANAR_MAP_H_
