// A stand-in for grid_map_msgs/GridMap with the fields GpuElevationMap fills (voxgraph_amd/cpp/gpu_elevation_map.h), so that
// the mirror can be compiled and run without ROS.  Field names and types are those of the ROS message (ROS 1).
#ifndef TESTS_CPP_GRID_MAP_STANDIN_H_
#define TESTS_CPP_GRID_MAP_STANDIN_H_

#include <cstdint>
#include <string>
#include <vector>

namespace grid_map_msgs_standin {

struct Point {
  double x = 0, y = 0, z = 0;
};
struct Quaternion {
  double x = 0, y = 0, z = 0, w = 1;
};
struct Pose {
  Point position;
  Quaternion orientation;
};
struct GridMapInfo {
  double resolution = 0;
  double length_x = 0, length_y = 0;
  Pose pose;  // the centre of the map
};
struct MultiArrayDimension {
  std::string label;
  uint32_t size = 0, stride = 0;
};
struct MultiArrayLayout {
  std::vector<MultiArrayDimension> dim;
  uint32_t data_offset = 0;
};
struct Float32MultiArray {
  MultiArrayLayout layout;
  std::vector<float> data;
};
struct GridMap {
  GridMapInfo info;
  std::vector<std::string> layers;
  std::vector<std::string> basic_layers;
  std::vector<Float32MultiArray> data;
  uint16_t outer_start_index = 0, inner_start_index = 0;
};

}  // namespace grid_map_msgs_standin

#endif  // TESTS_CPP_GRID_MAP_STANDIN_H_
