// Stand-in for visualization_msgs/Marker (with geometry_msgs/Point, Pose, Vector3 and std_msgs/ColorRGBA) with the members
// voxgraph_amd::DownloadMarker touches [recalled], for building and testing it without ROS.
#ifndef TESTS_CPP_MARKER_STANDIN_H_
#define TESTS_CPP_MARKER_STANDIN_H_

#include <cstdint>
#include <string>
#include <vector>

namespace standin_marker {

struct Header {
  uint32_t seq = 0;
  double stamp = 0;
  std::string frame_id;
};

struct Point {
  double x = 0, y = 0, z = 0;
};

struct Quaternion {
  double x = 0, y = 0, z = 0, w = 0;  // (a ROS message's numbers start at zero: w = 1 has to be written)
};

struct Pose {
  Point position;
  Quaternion orientation;
};

struct Vector3 {
  double x = 0, y = 0, z = 0;
};

struct ColorRGBA {
  float r = 0, g = 0, b = 0, a = 0;
};

struct Marker {
  enum : int32_t { ARROW = 0, CUBE = 1, SPHERE = 2, LINE_LIST = 5, TRIANGLE_LIST = 11 };
  enum : int32_t { ADD = 0, MODIFY = 0, DELETE = 2 };
  Header header;
  std::string ns;
  int32_t id = 0;
  int32_t type = 0;
  int32_t action = 0;
  Pose pose;
  Vector3 scale;
  ColorRGBA color;
  double lifetime = 0;
  uint8_t frame_locked = 0;
  std::vector<Point> points;
  std::vector<ColorRGBA> colors;
  std::string text;
  std::string mesh_resource;
  uint8_t mesh_use_embedded_materials = 0;
};

}  // namespace standin_marker

#endif  // TESTS_CPP_MARKER_STANDIN_H_
