// A stand-in for nav_msgs/OccupancyGrid with the fields GpuPlanarMap fills (voxgraph_amd/cpp/gpu_planar_map.h), so that the
// mirror can be compiled and run without ROS.  Field names and types are those of the ROS message.
#ifndef TESTS_CPP_OCCUPANCY_GRID_STANDIN_H_
#define TESTS_CPP_OCCUPANCY_GRID_STANDIN_H_

#include <cstdint>
#include <vector>

namespace nav_msgs_standin {

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
struct MapMetaData {
  float resolution = 0;
  uint32_t width = 0, height = 0;
  Pose origin;
};
struct OccupancyGrid {
  MapMetaData info;
  std::vector<int8_t> data;
};

}  // namespace nav_msgs_standin

#endif  // TESTS_CPP_OCCUPANCY_GRID_STANDIN_H_
