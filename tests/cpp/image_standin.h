// Stand-ins for sensor_msgs/Image and sensor_msgs/CameraInfo with the members
// voxgraph_amd::GpuDepthImageIntegrator reads, for building and testing it without ROS.
#ifndef TESTS_CPP_IMAGE_STANDIN_H_
#define TESTS_CPP_IMAGE_STANDIN_H_

#include <array>
#include <cstdint>
#include <string>
#include <vector>

namespace standin {

struct Image {
  uint32_t height = 0, width = 0;
  std::string encoding;
  uint8_t is_bigendian = 0;
  uint32_t step = 0;  // bytes per row
  std::vector<uint8_t> data;
};

struct CameraInfo {
  uint32_t height = 0, width = 0;
  std::string distortion_model;
  std::vector<double> D;
  std::array<double, 9> K{};   // (boost::array<double, 9> in the generated message)
  std::array<double, 9> R{};
  std::array<double, 12> P{};
};

}  // namespace standin

#endif  // TESTS_CPP_IMAGE_STANDIN_H_
