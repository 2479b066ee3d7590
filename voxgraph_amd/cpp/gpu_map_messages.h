// Host-side mirror of what voxgraph publishes about its map, and of the receiving end:
//   voxblox::serializeLayerAsMsg<TsdfVoxel>(layer, only_updated = false, &msg)  [recalled]   -> serializeLayerAsMsg
//   ProjectedMapServer::publishProjectedMap (projected_map_server.cpp:21-38)    -> projectedMapMsg (action kReset)
//   SubmapServer::publishSubmapTsdf / publishSubmapTsdfAndEsdf (submap_server.cpp:83-105, cblox serializeSubmapToMsg)
//                                                                               -> submapTsdfMsg / submapTsdfAndEsdfMsg
//   SubmapServer::publishSubmapSurfacePointcloud (submap_server.cpp:107-163)    -> submapSurfacePointcloud
//   voxblox::deserializeMsgToLayer(msg, layer) [recalled]                       -> deserializeMsgToLayer
// The device does the work (include/voxgraph_amd.h, "Map messages"); this header moves the result into message objects.
// No ROS, voxblox or cblox headers are needed: every function is templated on the message type and touches the members
// the real messages have [recalled] --
//   voxblox_msgs::Layer   voxel_size (f64), voxels_per_side, layer_type ("tsdf" / "esdf"), action, blocks[]
//   voxblox_msgs::Block   x_index, y_index, z_index, data[]
//   cblox_msgs::MapLayer  map_header, type, tsdf_layer, esdf_layer        (type: 0 TSDF, 1 TSDF + ESDF [recalled])
//   sensor_msgs::PointCloud2  height, width, fields[], is_bigendian, point_step, row_step, data, is_dense
// so they compile against the real messages and against stand-ins alike.  Headers, stamps and frame names are the
// caller's: whatever it has put into the message before the call stays there.
#ifndef VOXGRAPH_AMD_CPP_GPU_MAP_MESSAGES_H_
#define VOXGRAPH_AMD_CPP_GPU_MAP_MESSAGES_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "voxgraph_amd.h"

namespace voxgraph_amd {

// voxblox::MapDerializationAction [recalled]
enum class MapDerializationAction : uint8_t { kUpdate = VGX_MSG_ACTION_UPDATE, kMerge = VGX_MSG_ACTION_MERGE, kReset = VGX_MSG_ACTION_RESET };

class GpuMapMessages {
 public:
  static constexpr uint8_t kFloat32 = 7;        // sensor_msgs::PointField::FLOAT32
  static constexpr uint8_t kMapLayerTsdf = 0;   // cblox_msgs::MapLayer::TSDF [recalled]
  static constexpr uint8_t kMapLayerEsdf = 1;   // cblox_msgs::MapLayer::ESDF [recalled]: the TSDF and the ESDF layer

  explicit GpuMapMessages(vgx_ctx ctx) : ctx_(ctx) {
    if (vgx_map_msg_create(ctx, &msg_) != VGX_OK) throw std::runtime_error(std::string("vgx_map_msg_create: ") + vgx_last_error(ctx));
  }
  ~GpuMapMessages() { vgx_map_msg_destroy(msg_); }
  GpuMapMessages(const GpuMapMessages&) = delete;
  GpuMapMessages& operator=(const GpuMapMessages&) = delete;

  // serializeLayerAsMsg(layer, false, &msg) of a vgx_tsdf_layer (the active submap, the projected map); action kUpdate
  // as voxblox leaves it
  template <class LayerMsg>
  void serializeLayerAsMsg(vgx_tsdf_layer layer, LayerMsg* msg, MapDerializationAction action = MapDerializationAction::kUpdate) {
    check(vgx_tsdf_layer_serialize(layer, msg_), "vgx_tsdf_layer_serialize");
    fill(msg, action);
  }
  // ... of a finished submap's raw layer: which = VGX_EVAL_LAYER_TSDF / VGX_EVAL_LAYER_ESDF
  template <class LayerMsg>
  void serializeLayerAsMsg(vgx_submap submap, int32_t which, LayerMsg* msg, MapDerializationAction action = MapDerializationAction::kUpdate) {
    check(vgx_submap_serialize_layer(submap, which, msg_), "vgx_submap_serialize_layer");
    fill(msg, action);
  }

  // publishProjectedMap's message body: the projected map's TSDF layer with action kReset
  template <class MapLayerMsg>
  void projectedMapMsg(vgx_tsdf_layer projected_map, MapLayerMsg* msg) {
    msg->type = kMapLayerTsdf;
    serializeLayerAsMsg(projected_map, &msg->tsdf_layer, MapDerializationAction::kReset);
  }
  // publishSubmapTsdf's / publishSubmapTsdfAndEsdf's message body (cblox serializeSubmapToMsg: action kReset [recalled])
  template <class MapLayerMsg>
  void submapTsdfMsg(vgx_submap submap, MapLayerMsg* msg) {
    msg->type = kMapLayerTsdf;
    serializeLayerAsMsg(submap, VGX_EVAL_LAYER_TSDF, &msg->tsdf_layer, MapDerializationAction::kReset);
  }
  template <class MapLayerMsg>
  void submapTsdfAndEsdfMsg(vgx_submap submap, MapLayerMsg* msg) {
    msg->type = kMapLayerEsdf;
    serializeLayerAsMsg(submap, VGX_EVAL_LAYER_TSDF, &msg->tsdf_layer, MapDerializationAction::kReset);
    serializeLayerAsMsg(submap, VGX_EVAL_LAYER_ESDF, &msg->esdf_layer, MapDerializationAction::kReset);
  }

  // T_B_S = T_S_B.inverse() as the row-major 3 x 4 affine of transformKindrToEigen, from T_S_B {qw,qx,qy,qz, tx,ty,tz}
  // (submap.getPoseHistory().begin()->second): conjugate quaternion, Eigen's toRotationMatrix, translation -(R t), in f32
  static void inversePoseAffine(const float T_S_B[7], float T_B_S[12]) {
    const float w = T_S_B[0], x = -T_S_B[1], y = -T_S_B[2], z = -T_S_B[3];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float R[9] = {1.0f - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0f - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                        1.0f - (txx + tyy)};
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T_B_S[4 * r + c] = R[3 * r + c];
      T_B_S[4 * r + 3] = -((R[3 * r] * T_S_B[4] + R[3 * r + 1] * T_S_B[5]) + R[3 * r + 2] * T_S_B[6]);
    }
  }

  // publishSubmapSurfacePointcloud's PointCloud2 (a pcl::PointXYZI cloud through pcl::toROSMsg): the submap's isosurface
  // points with intensity = weight, moved into the base_link frame by T_B_S when fake_6dof_transforms is set.
  // T_S_B: the first pose of the submap's pose history {qw,qx,qy,qz, tx,ty,tz}; not read when the switch is off.
  template <class PointCloud2Msg>
  void submapSurfacePointcloud(vgx_submap submap, bool fake_6dof_transforms, const float T_S_B[7], PointCloud2Msg* cloud,
                               int32_t point_type = VGX_POINTS_ISOSURFACE) {
    float T[12];
    if (fake_6dof_transforms) {
      if (!T_S_B) throw std::invalid_argument("submapSurfacePointcloud: fake_6dof_transforms without a pose");
      inversePoseAffine(T_S_B, T);
    }
    check(vgx_submap_surface_msg(submap, point_type, fake_6dof_transforms ? T : nullptr, msg_), "vgx_submap_surface_msg");
    int64_t n = 0, n_bytes = 0;
    vgx_map_msg_stats(msg_, nullptr, &n, nullptr, &n_bytes);
    if (n > 0x7fffffff / 32) throw std::length_error("submapSurfacePointcloud: more points than a PointCloud2 row holds");
    cloud->height = 1;
    cloud->width = (uint32_t)n;
    cloud->is_bigendian = 0;
    cloud->point_step = 32;
    cloud->row_step = (uint32_t)(32 * n);
    cloud->is_dense = 1;
    static const char* const names[4] = {"x", "y", "z", "intensity"};
    static const uint32_t offsets[4] = {0, 4, 8, 16};
    cloud->fields.resize(4);
    for (int k = 0; k < 4; ++k) {
      cloud->fields[k].name = names[k];
      cloud->fields[k].offset = offsets[k];
      cloud->fields[k].datatype = kFloat32;
      cloud->fields[k].count = 1;
    }
    cloud->data.resize((size_t)n_bytes);
    check(vgx_map_msg_download(msg_, nullptr, cloud->data.data()), "vgx_map_msg_download");
  }

  // deserializeMsgToLayer(msg, layer): false where voxblox returns false (a message that does not fit the layer, an
  // unknown action, a block whose data has the wrong length); the action is the message's
  template <class LayerMsg>
  bool deserializeMsgToLayer(const LayerMsg& msg, vgx_tsdf_layer layer) {
    return deserializeMsgToLayer(msg, static_cast<MapDerializationAction>(msg.action), layer);
  }
  template <class LayerMsg>
  bool deserializeMsgToLayer(const LayerMsg& msg, MapDerializationAction action, vgx_tsdf_layer layer) {
    const size_t n = msg.blocks.size();
    const size_t per_block = (size_t)msg.voxels_per_side * msg.voxels_per_side * msg.voxels_per_side * 3;
    index_.resize(3 * n);
    words_.resize(n * per_block);
    for (size_t b = 0; b < n; ++b) {
      const auto& blk = msg.blocks[b];
      if (blk.data.size() != per_block) return false;
      index_[3 * b] = blk.x_index;
      index_[3 * b + 1] = blk.y_index;
      index_[3 * b + 2] = blk.z_index;
      std::memcpy(words_.data() + b * per_block, blk.data.data(), per_block * 4);
    }
    const std::string type = msg.layer_type;
    const int rc = vgx_tsdf_layer_deserialize(layer, (int32_t)action, type == "tsdf" ? VGX_EVAL_LAYER_TSDF : VGX_EVAL_LAYER_ESDF,
                                              (double)msg.voxel_size, (int32_t)msg.voxels_per_side, (int32_t)n, index_.data(),
                                              words_.data(), (int64_t)words_.size());
    if (rc == VGX_ERR_INVALID) return false;
    check(rc, "vgx_tsdf_layer_deserialize");
    return true;
  }

  vgx_map_msg handle() const { return msg_; }

 private:
  void check(int rc, const char* what) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string(what) + ": " + vgx_last_error(ctx_));
  }
  // the handle's layer message -> msg
  template <class LayerMsg>
  void fill(LayerMsg* msg, MapDerializationAction action) {
    int32_t kind = 0, words_per_voxel = 0, vps = 0;
    int64_t n = 0, n_bytes = 0;
    float voxel_size = 0;
    vgx_map_msg_stats(msg_, &kind, &n, &words_per_voxel, &n_bytes);
    check(vgx_map_msg_layer_geometry(msg_, &voxel_size, &vps), "vgx_map_msg_layer_geometry");
    msg->voxel_size = voxel_size;
    msg->voxels_per_side = (uint32_t)vps;
    msg->layer_type = kind == VGX_MSG_ESDF_LAYER ? "esdf" : "tsdf";
    msg->action = static_cast<uint8_t>(action);
    index_.resize(3 * (size_t)n);
    words_.resize((size_t)n_bytes / 4);
    check(vgx_map_msg_download(msg_, index_.data(), words_.data()), "vgx_map_msg_download");
    const size_t per_block = n > 0 ? words_.size() / (size_t)n : 0;
    msg->blocks.resize((size_t)n);
    for (size_t b = 0; b < (size_t)n; ++b) {
      auto& blk = msg->blocks[b];
      blk.x_index = index_[3 * b];
      blk.y_index = index_[3 * b + 1];
      blk.z_index = index_[3 * b + 2];
      blk.data.assign(words_.begin() + b * per_block, words_.begin() + (b + 1) * per_block);
    }
  }

  vgx_ctx ctx_;
  vgx_map_msg msg_ = nullptr;
  std::vector<int32_t> index_;
  std::vector<uint32_t> words_;
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_MAP_MESSAGES_H_
