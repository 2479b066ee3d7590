// voxgraph_amd::GpuMapMessages (voxgraph_amd/cpp/gpu_map_messages.h) end to end on stand-in message types
// (map_msgs_standin.h), from plain C++.
//   map_msg_smoke compile        no device: the header instantiates on the stand-ins, inversePoseAffine by hand
//   map_msg_smoke IN OUT         IN: a layer with colours, an ESDF over its blocks, a pose, points with weights
//                                OUT: the projected-map message's words, the layer deserialised from it, the submap
//                                message's TSDF and ESDF words, and the surface cloud with the T_B_S it was moved by
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gpu_map_messages.h"
#include "gpu_pointcloud_integrator.h"
#include "map_msgs_standin.h"

using voxgraph_amd::GpuMapMessages;
using voxgraph_amd::MapDerializationAction;

namespace {

template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return n == 0 || fread(p, sizeof(T), n, f) == n;
}
template <class T>
void wr(FILE* f, const T* p, size_t n) {
  if (n) fwrite(p, sizeof(T), n, f);
}

void write_layer_msg(FILE* out, const standin_map::Layer& l) {
  const uint32_t n = (uint32_t)l.blocks.size(), action = l.action, esdf = l.layer_type == "esdf";
  wr(out, &n, 1);
  wr(out, &action, 1);
  wr(out, &esdf, 1);
  wr(out, &l.voxels_per_side, 1);
  wr(out, &l.voxel_size, 1);
  for (const auto& b : l.blocks) {
    const int32_t i[3] = {b.x_index, b.y_index, b.z_index};
    wr(out, i, 3);
  }
  for (const auto& b : l.blocks) wr(out, b.data.data(), b.data.size());
}

int compile_checks() {
  // the identity, and a quarter turn about z with a translation: T_B_S = T_S_B.inverse()
  float T[12];
  const float id[7] = {1, 0, 0, 0, 0, 0, 0};
  GpuMapMessages::inversePoseAffine(id, T);
  const float want_id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int k = 0; k < 12; ++k)
    if (T[k] != want_id[k] && !(T[k] == 0.0f && want_id[k] == 0.0f)) return 10;
  const float s = std::sqrt(0.5f), quarter[7] = {s, 0, 0, s, 1, 2, 3};  // x -> y; inverse: y -> x, t' = -(R^T t) = (-2, 1, -3)
  GpuMapMessages::inversePoseAffine(quarter, T);
  const float want[12] = {0, 1, 0, -2, -1, 0, 0, 1, 0, 0, 1, -3};
  for (int k = 0; k < 12; ++k)
    if (std::fabs(T[k] - want[k]) > 1e-6f) return 11;
  if ((int)MapDerializationAction::kUpdate != 0 || (int)MapDerializationAction::kMerge != 1 || (int)MapDerializationAction::kReset != 2) return 12;
  if (standin_map::Layer::ACTION_RESET != VGX_MSG_ACTION_RESET || standin_map::MapLayer::ESDF != GpuMapMessages::kMapLayerEsdf) return 13;
  // the member functions instantiate on the stand-ins (taken by address: nothing runs without a device)
  auto f1 = &GpuMapMessages::projectedMapMsg<standin_map::MapLayer>;
  auto f2 = &GpuMapMessages::submapTsdfMsg<standin_map::MapLayer>;
  auto f3 = &GpuMapMessages::submapTsdfAndEsdfMsg<standin_map::MapLayer>;
  auto f4 = &GpuMapMessages::submapSurfacePointcloud<standin_map::PointCloud2>;
  bool (GpuMapMessages::*f5)(const standin_map::Layer&, vgx_tsdf_layer) = &GpuMapMessages::deserializeMsgToLayer<standin_map::Layer>;
  if (!f1 || !f2 || !f3 || !f4 || !f5) return 14;
  printf("MAP_MSG_COMPILE_OK\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "compile") == 0) return compile_checks();
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t vps = 0, nb = 0, np = 0;
  float vs = 0, pose[7];
  if (!rd(in, &vps, 1) || !rd(in, &nb, 1) || !rd(in, &np, 1) || !rd(in, &vs, 1) || !rd(in, pose, 7)) return 3;
  const size_t vox = (size_t)vps * vps * vps, nv = (size_t)nb * vox;
  std::vector<int32_t> bi(3 * (size_t)nb);
  std::vector<float> d(nv), w(nv), ed(nv), xyz(3 * (size_t)np), pw((size_t)np), pd((size_t)np, 0.0f);
  std::vector<uint8_t> rgba(4 * nv), eo(nv);
  if (!rd(in, bi.data(), bi.size()) || !rd(in, d.data(), nv) || !rd(in, w.data(), nv) || !rd(in, rgba.data(), 4 * nv) ||
      !rd(in, ed.data(), nv) || !rd(in, eo.data(), nv) || !rd(in, xyz.data(), xyz.size()) || !rd(in, pw.data(), pw.size()))
    return 3;
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 7;
  try {
    GpuMapMessages messages(ctx);
    voxgraph_amd::GpuTsdfLayer projected(ctx, vs, vps), received(ctx, vs, vps);
    if (vgx_tsdf_layer_upload(projected.handle(), nb, bi.data(), d.data(), w.data(), rgba.data()) != VGX_OK) return 5;
    // 1. the projected-map message, with a header the call must leave alone
    standin_map::MapLayer map_msg;
    map_msg.header.frame_id = "mission";
    map_msg.header.stamp = 12.5;
    map_msg.map_header.id = 7;
    messages.projectedMapMsg(projected.handle(), &map_msg);
    if (map_msg.header.frame_id != "mission" || map_msg.header.stamp != 12.5 || map_msg.map_header.id != 7) return 20;
    if (map_msg.type != standin_map::MapLayer::TSDF || map_msg.tsdf_layer.action != standin_map::Layer::ACTION_RESET ||
        map_msg.tsdf_layer.layer_type != "tsdf" || !map_msg.esdf_layer.blocks.empty())
      return 21;
    write_layer_msg(out, map_msg.tsdf_layer);
    // 2. the receiving end: something to reset, then the message's own action
    const int32_t junk_bi[3] = {bi.empty() ? 0 : bi[0] + 9, 1, 2};
    std::vector<float> ones(vox, 1.0f);
    std::vector<uint8_t> grey(4 * vox, 77);
    if (vgx_tsdf_layer_upload(received.handle(), 1, junk_bi, ones.data(), ones.data(), grey.data()) != VGX_OK) return 5;
    if (!messages.deserializeMsgToLayer(map_msg.tsdf_layer, received.handle())) return 22;
    // what voxblox answers false to: another geometry, an ESDF layer, a short block
    standin_map::Layer bad = map_msg.tsdf_layer;
    bad.voxels_per_side = vps == 8 ? 16 : 8;
    if (messages.deserializeMsgToLayer(bad, received.handle())) return 23;
    bad = map_msg.tsdf_layer;
    bad.layer_type = "esdf";
    if (messages.deserializeMsgToLayer(bad, received.handle())) return 24;
    bad = map_msg.tsdf_layer;
    if (!bad.blocks.empty()) {
      bad.blocks[0].data.pop_back();
      if (messages.deserializeMsgToLayer(bad, received.handle())) return 25;
    }
    int32_t nr = received.getNumberOfAllocatedBlocks();
    std::vector<int32_t> rbi(3 * (size_t)nr);
    std::vector<float> rd_(nr * vox), rw(nr * vox);
    std::vector<uint8_t> rc(4 * nr * vox);
    if (vgx_tsdf_layer_download(received.handle(), rbi.data(), rd_.data(), rw.data(), rc.data()) != VGX_OK) return 6;
    wr(out, &nr, 1);
    wr(out, rbi.data(), rbi.size());
    wr(out, rd_.data(), rd_.size());
    wr(out, rw.data(), rw.size());
    wr(out, rc.data(), rc.size());
    // 3. the submap messages
    vgx_submap sm = nullptr;
    if (vgx_submap_create(ctx, 7, vs, vps, nb, bi.data(), d.data(), w.data(), ed.data(), eo.data(), &sm) != VGX_OK) return 5;
    standin_map::MapLayer tsdf_msg, both_msg;
    messages.submapTsdfMsg(sm, &tsdf_msg);
    messages.submapTsdfAndEsdfMsg(sm, &both_msg);
    if (tsdf_msg.type != standin_map::MapLayer::TSDF || both_msg.type != standin_map::MapLayer::ESDF || !tsdf_msg.esdf_layer.blocks.empty() ||
        both_msg.esdf_layer.layer_type != "esdf" || both_msg.esdf_layer.action != standin_map::Layer::ACTION_RESET)
      return 26;
    write_layer_msg(out, tsdf_msg.tsdf_layer);
    write_layer_msg(out, both_msg.tsdf_layer);
    write_layer_msg(out, both_msg.esdf_layer);
    // 4. the surface cloud, as it is and moved by T_B_S
    if (vgx_submap_set_points(sm, VGX_POINTS_ISOSURFACE, np, xyz.data(), pd.data(), pw.data(), VGX_POINTS_KEEP_ORDER) != VGX_OK) return 5;
    float T[12];
    GpuMapMessages::inversePoseAffine(pose, T);
    wr(out, T, 12);
    for (int fake = 0; fake < 2; ++fake) {
      standin_map::PointCloud2 cloud;
      cloud.header.frame_id = "imu";
      messages.submapSurfacePointcloud(sm, fake != 0, pose, &cloud);
      if (cloud.header.frame_id != "imu" || cloud.height != 1 || cloud.width != (uint32_t)np || cloud.point_step != 32 ||
          cloud.row_step != 32u * (uint32_t)np || cloud.is_bigendian != 0 || cloud.is_dense != 1 || cloud.fields.size() != 4 ||
          cloud.data.size() != 32 * (size_t)np)
        return 27;
      // the scan side's own field detection accepts it: x y z FLOAT32 at 0 / 4 / 8, intensity FLOAT32 at 16
      const vgx_scan_layout l = voxgraph_amd::GpuPointcloudIntegrator::layoutOf(cloud);
      if (l.offset_x != 0 || l.offset_y != 4 || l.offset_z != 8 || l.color_kind != VGX_SCAN_COLOR_INTENSITY || l.color_offset != 16 ||
          vgx_scan_layout_check(&l, (int64_t)cloud.data.size()) != VGX_OK)
        return 28;
      wr(out, cloud.data.data(), cloud.data.size());
    }
    vgx_submap_destroy(sm);
  } catch (const std::exception& e) {
    fprintf(stderr, "%s\n", e.what());
    return 8;
  }
  fclose(out);
  vgx_ctx_destroy(ctx);
  printf("MAP_MSG_SMOKE_OK\n");
  return 0;
}
