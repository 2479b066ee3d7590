// Stand-ins for voxblox_msgs/Layer, voxblox_msgs/Block, cblox_msgs/MapLayer, cblox_msgs/MapHeader and
// sensor_msgs/PointCloud2 with the members voxgraph_amd::GpuMapMessages touches [recalled], for building and testing it
// without ROS.  The PointCloud2 has the shape of tests/cpp/pointcloud2_standin.h's.
#ifndef TESTS_CPP_MAP_MSGS_STANDIN_H_
#define TESTS_CPP_MAP_MSGS_STANDIN_H_

#include <cstdint>
#include <string>
#include <vector>

namespace standin_map {

struct Block {
  int32_t x_index = 0, y_index = 0, z_index = 0;
  std::vector<uint32_t> data;
};

struct Layer {
  enum : uint8_t { ACTION_UPDATE = 0, ACTION_MERGE = 1, ACTION_RESET = 2 };
  double voxel_size = 0;
  uint32_t voxels_per_side = 0;
  std::string layer_type;
  uint8_t action = 0;
  std::vector<Block> blocks;
};

struct Header {
  uint32_t seq = 0;
  double stamp = 0;
  std::string frame_id;
};

struct MapHeader {
  Header header;
  uint32_t id = 0;
  uint8_t is_submap = 0;
};

struct MapLayer {
  enum : uint8_t { TSDF = 0, ESDF = 1 };
  Header header;
  MapHeader map_header;
  uint8_t type = 0;
  Layer tsdf_layer, esdf_layer;
};

struct PointField {
  enum : uint8_t { INT8 = 1, UINT8 = 2, INT16 = 3, UINT16 = 4, INT32 = 5, UINT32 = 6, FLOAT32 = 7, FLOAT64 = 8 };
  std::string name;
  uint32_t offset = 0;
  uint8_t datatype = 0;
  uint32_t count = 0;
};

struct PointCloud2 {
  Header header;
  uint32_t height = 0, width = 0;
  std::vector<PointField> fields;
  uint8_t is_bigendian = 0;
  uint32_t point_step = 0, row_step = 0;
  std::vector<uint8_t> data;
  uint8_t is_dense = 0;
};

}  // namespace standin_map

#endif  // TESTS_CPP_MAP_MSGS_STANDIN_H_
