// The elevation map for a legged or rough-terrain planner: a layer's height band as a grid_map_msgs/GridMap.
//
// voxgraph's own demo robot walks; a footstep or rough-terrain planner steers through a 2.5D grid of named layers.
// GpuElevationMap fills one from a device layer -- a vgx_tsdf_layer (the active submap, the projected map) or a finished
// vgx_submap's raw TSDF or ESDF layer -- in one call; the column walk, the step window, the slope, the class and the
// distance transform run on the device (vgx_elevation.hip), and what crosses to the host is the grid.  Rules (column,
// outputs, step, gradient, class, distance): include/voxgraph_amd.h, "Elevation map".
//
// ROS is not a dependency: the message type is a template parameter, and anything with grid_map_msgs/GridMap's fields --
// info.resolution, info.length_x, info.length_y, info.pose.position.{x, y, z}, layers and basic_layers (std::vector<
// std::string>), data (a std::vector of Float32MultiArray: layout.dim[] {label, size, stride}, data std::vector<float>) --
// will do (tests/cpp/grid_map_standin.h is the one the tests use).  The header is the caller's.
//
// Cell order.  Every layer is written in THIS library's grid order, row-major with x fastest from the corner
// (x0 * voxel_size, y0 * voxel_size): data[iy * W + ix], and layout.dim says so ("row_index" = H first, "column_index" = W).
// grid_map's own Eigen storage runs from the opposite corner; a caller that hands the message to grid_map::
// GridMapRosConverter flips both axes first.
#ifndef VOXGRAPH_AMD_CPP_GPU_ELEVATION_MAP_H_
#define VOXGRAPH_AMD_CPP_GPU_ELEVATION_MAP_H_

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "voxgraph_amd.h"

namespace voxgraph_amd {

// vgx_elevation_map_config_default() with the band set: there is no default band
inline vgx_elevation_map_config ElevationMapConfig(float z_min, float z_max) {
  vgx_elevation_map_config cfg;
  vgx_elevation_map_config_default(&cfg);
  cfg.z_min = z_min;
  cfg.z_max = z_max;
  return cfg;
}

// A vgx_elevation_map owned for the length of a scope (reuse one across calls: its device buffers grow on demand).
class GpuElevationMap {
 public:
  explicit GpuElevationMap(vgx_ctx ctx) : ctx_(ctx) {
    if (vgx_elevation_map_create(ctx, &h_) != VGX_OK)
      throw std::runtime_error(std::string("vgx_elevation_map_create: ") + vgx_last_error(ctx));
  }
  GpuElevationMap(const GpuElevationMap&) = delete;
  GpuElevationMap& operator=(const GpuElevationMap&) = delete;
  ~GpuElevationMap() {
    if (h_) vgx_elevation_map_destroy(h_);
  }
  vgx_elevation_map handle() const { return h_; }

  // the producing calls: the map is complete when they return
  void update(vgx_tsdf_layer layer, const vgx_elevation_map_config& cfg) { check(vgx_tsdf_layer_elevation_map(layer, &cfg, h_)); }
  void update(vgx_submap submap, int32_t layer, const vgx_elevation_map_config& cfg) {
    check(vgx_submap_layer_elevation_map(submap, layer, &cfg, h_));
  }

  int32_t width() const { return dim(0); }
  int32_t height() const { return dim(1); }
  // cells in state 0 (unknown), 1 (surface), 2 (hole), 3 (blocked); in class 0 (unknown), 1 (traversable), 2 (not)
  void counts(int64_t states[4], int64_t classes[3]) const {
    check(vgx_elevation_map_stats(h_, nullptr, nullptr, nullptr, states, classes));
  }

  // The grid as a GridMap of six f32 layers, NaN where a layer has no value (grid_map's convention):
  //   elevation        the surface height (metres, the layer's frame); NaN where the cell has no surface
  //   slope            rise over run; NaN where it is undefined
  //   step             max - min of the surface heights in the window (metres); NaN where the cell has no surface
  //   headroom         free height above the surface (metres: voxels * voxel_size); NaN where the cell has no surface
  //   traversability   the class: 0 unknown, 1 traversable, 2 not traversable
  //   distance         planar distance to the nearest obstacle cell (metres, clipped to max_distance_m)
  // basic_layers = {"elevation"}.  info.pose.position is the centre of the map, at height `z`.
  template <class GridMapT>
  void toGridMap(GridMapT* msg, double z = 0.0) const {
    int32_t mn[2], dm[2];
    float vs = 0.0f;
    check(vgx_elevation_map_stats(h_, mn, dm, &vs, nullptr, nullptr));
    const size_t n = static_cast<size_t>(dm[0]) * static_cast<size_t>(dm[1]);
    msg->info.resolution = vs;
    msg->info.length_x = static_cast<double>(dm[0]) * vs;
    msg->info.length_y = static_cast<double>(dm[1]) * vs;
    msg->info.pose.position.x = (static_cast<double>(mn[0]) + 0.5 * dm[0]) * vs;
    msg->info.pose.position.y = (static_cast<double>(mn[1]) + 0.5 * dm[1]) * vs;
    msg->info.pose.position.z = z;
    static const char* const kLayers[6] = {"elevation", "slope", "step", "headroom", "traversability", "distance"};
    msg->layers.assign(kLayers, kLayers + 6);
    msg->basic_layers.assign(1, "elevation");
    msg->data.resize(6);
    for (auto& layer : msg->data) {
      layer.layout.dim.resize(2);
      layer.layout.dim[0].label = "row_index";
      layer.layout.dim[0].size = static_cast<uint32_t>(dm[1]);
      layer.layout.dim[0].stride = static_cast<uint32_t>(n);
      layer.layout.dim[1].label = "column_index";
      layer.layout.dim[1].size = static_cast<uint32_t>(dm[0]);
      layer.layout.dim[1].stride = static_cast<uint32_t>(dm[0]);
      layer.data.resize(n);
    }
    std::vector<uint8_t> state(n), slope_valid(n), cls(n);
    std::vector<int32_t> headroom(n);
    check(vgx_elevation_map_download(h_, state.data(), msg->data[0].data.data(), headroom.data(), nullptr, nullptr, msg->data[2].data.data(),
                                     nullptr, msg->data[1].data.data(), slope_valid.data(), cls.data(), msg->data[5].data.data()));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < n; ++i) {
      const bool surface = state[i] == 1;
      if (!surface) msg->data[0].data[i] = msg->data[2].data[i] = nan;
      if (!slope_valid[i]) msg->data[1].data[i] = nan;
      msg->data[3].data[i] = surface ? static_cast<float>(headroom[i]) * vs : nan;
      msg->data[4].data[i] = static_cast<float>(cls[i]);
    }
  }

 private:
  int32_t dim(int a) const {
    int32_t dm[2] = {0, 0};
    check(vgx_elevation_map_stats(h_, nullptr, dm, nullptr, nullptr, nullptr));
    return dm[a];
  }
  void check(int rc) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string("elevation map: ") + vgx_last_error(ctx_));
  }
  vgx_ctx ctx_;
  vgx_elevation_map h_ = nullptr;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_ELEVATION_MAP_H_
