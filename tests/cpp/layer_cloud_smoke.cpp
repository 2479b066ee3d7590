// The layer point clouds (voxgraph_amd/cpp/gpu_layer_pointcloud.h) from plain C++: voxblox_ros' create...Pointcloud...
// functions over a vgx_tsdf_layer, a finished submap and the error layer of an evaluation, their outputs written for
// tests/test_layer_cloud_cpp.py to compare with the Python path.
//   layer_cloud_smoke IN OUT
// IN: int32 vps, n_blocks; f32 voxel_size, surface_distance, slice_value; int32 slice_axis; int32 block_index [nb][3];
//     f32 tsdf_d, tsdf_w, esdf_d [nb][vps^3]; u8 esdf_o [nb][vps^3]; u8 rgba [nb][vps^3][4]; then a second submap (the
//     evaluation's test side) on its own blocks: int32 n_blocks; block_index; f32 esdf_d; u8 esdf_o
// OUT, each cloud as int64 n then n records: layer distance, layer surface distance, layer surface colour (16-byte
//     PointXYZRGBA), layer slice; submap TSDF surface distance, submap ESDF distance, submap ESDF slice; the error layer's
//     distance cloud and slice; last the two evaluations' details (bytes)
#include <cstdio>
#include <vector>

#include "gpu_layer_pointcloud.h"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}
template <class T>
void wr(FILE* f, const std::vector<T>& v) {
  const int64_t n = (int64_t)v.size();
  fwrite(&n, 8, 1, f);
  fwrite(v.data(), sizeof(T), v.size(), f);
}
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(voxgraph_amd::PointXYZI) == 16 && sizeof(voxgraph_amd::PointXYZRGBA) == 16, "16-byte points");
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t vps = 0, nb = 0, axis = 0;
  float vs = 0, sd = 0, plane = 0;
  if (!rd(in, &vps, 1) || !rd(in, &nb, 1) || !rd(in, &vs, 1) || !rd(in, &sd, 1) || !rd(in, &plane, 1) || !rd(in, &axis, 1)) return 3;
  const size_t vox = (size_t)vps * vps * vps, nv = (size_t)nb * vox;
  std::vector<int32_t> bi(3 * (size_t)nb);
  std::vector<float> td(nv), tw(nv), ed(nv);
  std::vector<uint8_t> eo(nv), rgba(4 * nv);
  if (!rd(in, bi.data(), bi.size()) || !rd(in, td.data(), nv) || !rd(in, tw.data(), nv) || !rd(in, ed.data(), nv) ||
      !rd(in, eo.data(), nv) || !rd(in, rgba.data(), 4 * nv))
    return 3;
  int32_t nb2 = 0;
  if (!rd(in, &nb2, 1)) return 3;
  const size_t nv2 = (size_t)nb2 * vox;
  std::vector<int32_t> bi2(3 * (size_t)nb2);
  std::vector<float> ed2(nv2);
  std::vector<uint8_t> eo2(nv2);
  if (!rd(in, bi2.data(), bi2.size()) || !rd(in, ed2.data(), nv2) || !rd(in, eo2.data(), nv2)) return 3;
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  vgx_submap sm = nullptr, test = nullptr;
  vgx_tsdf_layer layer = nullptr;
  if (vgx_submap_create(ctx, 0, vs, vps, nb, bi.data(), td.data(), tw.data(), ed.data(), eo.data(), &sm) != VGX_OK) return 5;
  if (vgx_submap_create(ctx, 1, vs, vps, nb2, bi2.data(), ed2.data(), ed2.data(), ed2.data(), eo2.data(), &test) != VGX_OK) return 5;
  if (vgx_tsdf_layer_create(ctx, vs, vps, nullptr, nullptr, 0, &layer) != VGX_OK) return 5;
  if (vgx_tsdf_layer_upload(layer, nb, bi.data(), td.data(), tw.data(), rgba.data()) != VGX_OK) return 5;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  try {
    using namespace voxgraph_amd;
    std::vector<PointXYZI> cloud;
    std::vector<PointXYZRGBA> coloured;
    createDistancePointcloudFromTsdfLayer(ctx, layer, &cloud);
    wr(out, cloud);
    createSurfaceDistancePointcloudFromTsdfLayer(ctx, layer, sd, &cloud);
    wr(out, cloud);
    createSurfacePointcloudFromTsdfLayer(ctx, layer, sd, &coloured);
    wr(out, coloured);
    createDistancePointcloudFromTsdfLayerSlice(ctx, layer, (unsigned)axis, plane, &cloud);
    wr(out, cloud);
    createSurfaceDistancePointcloudFromTsdfLayer(ctx, sm, sd, &cloud);
    wr(out, cloud);
    createDistancePointcloudFromEsdfLayer(ctx, sm, &cloud);
    wr(out, cloud);
    createDistancePointcloudFromEsdfLayerSlice(ctx, sm, (unsigned)axis, plane, &cloud);
    wr(out, cloud);
    // map_evaluation.cpp:90-106 without an error layer on the host
    const vgx_voxel_evaluation_details full = EvaluateLayersRmseWithCloudOnGpu(
        ctx, sm, test, VGX_EVAL_LAYER_ESDF, VGX_EVAL_IGNORE_BEHIND_TEST, LayerCloudConfig(VGX_CLOUD_DISTANCE), &cloud);
    wr(out, cloud);
    const vgx_voxel_evaluation_details slice = EvaluateLayersRmseWithCloudOnGpu(
        ctx, sm, test, VGX_EVAL_LAYER_ESDF, VGX_EVAL_IGNORE_BEHIND_TEST, LayerCloudConfig(VGX_CLOUD_DISTANCE, 0.6, axis, plane), &cloud);
    wr(out, cloud);
    fwrite(&full, sizeof(full), 1, out);
    fwrite(&slice, sizeof(slice), 1, out);
  } catch (const std::exception& e) {
    std::printf("FAILED %s\n", e.what());
    return 6;
  }
  fclose(out);
  vgx_tsdf_layer_destroy(layer);
  vgx_submap_destroy(test);
  vgx_submap_destroy(sm);
  vgx_ctx_destroy(ctx);
  std::printf("LAYER_CLOUD_SMOKE_OK\n");
  return 0;
}
