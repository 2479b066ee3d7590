// A stand-in for sensor_msgs/PointCloud2 and sensor_msgs/PointField with the members
// voxgraph_amd::GpuPointcloudIntegrator reads, for building and testing it without ROS.
#ifndef TESTS_CPP_POINTCLOUD2_STANDIN_H_
#define TESTS_CPP_POINTCLOUD2_STANDIN_H_

#include <cstdint>
#include <string>
#include <vector>

namespace standin {

struct PointField {
  enum : uint8_t { INT8 = 1, UINT8 = 2, INT16 = 3, UINT16 = 4, INT32 = 5, UINT32 = 6, FLOAT32 = 7, FLOAT64 = 8 };
  std::string name;
  uint32_t offset = 0;
  uint8_t datatype = 0;
  uint32_t count = 0;
};

struct PointCloud2 {
  uint32_t height = 0, width = 0;
  std::vector<PointField> fields;
  uint8_t is_bigendian = 0;  // (a bool in the message definition; ROS generates uint8_t)
  uint32_t point_step = 0, row_step = 0;
  std::vector<uint8_t> data;
  uint8_t is_dense = 0;
};

}  // namespace standin

#endif  // TESTS_CPP_POINTCLOUD2_STANDIN_H_
