// The planar map (voxgraph_amd/cpp/gpu_planar_map.h) from plain C++: an OccupancyGrid stand-in and the distance field of
// a vgx_tsdf_layer and of a finished submap's two layers, written for tests/test_planar_map_cpp.py to compare with the
// Python path.
//   planar_map_smoke IN OUT
// IN: int32 vps, n_blocks; f32 voxel_size; the vgx_planar_map_config (bytes); int32 block_index [nb][3]; f32 tsdf_d, tsdf_w,
//     esdf_d [nb][vps^3]; u8 esdf_o [nb][vps^3]
// OUT, per source (layer, submap TSDF, submap ESDF): f32 resolution; u32 width, height; f64 origin x, y, z; int64 counts [3];
//     i8 data [h][w]; f32 distance, clearance, obstacle height [h][w]
#include <cstdio>
#include <vector>

#include "gpu_planar_map.h"
#include "occupancy_grid_standin.h"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}
void wr(FILE* out, const voxgraph_amd::GpuPlanarMap& map, double z) {
  nav_msgs_standin::OccupancyGrid grid;
  map.toOccupancyGrid(&grid, z);
  const std::vector<float> distance = map.distanceField();
  std::vector<float> clearance, top;
  map.columns(&clearance, &top);
  int64_t counts[3];
  map.counts(counts);
  fwrite(&grid.info.resolution, 4, 1, out);
  fwrite(&grid.info.width, 4, 1, out);
  fwrite(&grid.info.height, 4, 1, out);
  fwrite(&grid.info.origin.position.x, 8, 1, out);
  fwrite(&grid.info.origin.position.y, 8, 1, out);
  fwrite(&grid.info.origin.position.z, 8, 1, out);
  fwrite(counts, 8, 3, out);
  fwrite(grid.data.data(), 1, grid.data.size(), out);
  fwrite(distance.data(), 4, distance.size(), out);
  fwrite(clearance.data(), 4, clearance.size(), out);
  fwrite(top.data(), 4, top.size(), out);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t vps = 0, nb = 0;
  float vs = 0;
  vgx_planar_map_config cfg;
  if (!rd(in, &vps, 1) || !rd(in, &nb, 1) || !rd(in, &vs, 1) || !rd(in, &cfg, 1)) return 3;
  const size_t nv = (size_t)nb * vps * vps * vps;
  std::vector<int32_t> bi(3 * (size_t)nb);
  std::vector<float> td(nv), tw(nv), ed(nv);
  std::vector<uint8_t> eo(nv);
  if (!rd(in, bi.data(), bi.size()) || !rd(in, td.data(), nv) || !rd(in, tw.data(), nv) || !rd(in, ed.data(), nv) || !rd(in, eo.data(), nv))
    return 3;
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  vgx_submap sm = nullptr;
  vgx_tsdf_layer layer = nullptr;
  if (vgx_submap_create(ctx, 0, vs, vps, nb, bi.data(), td.data(), tw.data(), ed.data(), eo.data(), &sm) != VGX_OK) return 5;
  if (vgx_tsdf_layer_create(ctx, vs, vps, nullptr, nullptr, 0, &layer) != VGX_OK) return 5;
  if (vgx_tsdf_layer_upload(layer, nb, bi.data(), td.data(), tw.data(), nullptr) != VGX_OK) return 5;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  try {
    using namespace voxgraph_amd;
    const double z = 0.5 * ((double)cfg.z_min + (double)cfg.z_max);
    GpuPlanarMap map(ctx);  // one handle, reused
    // a config built the C++ way gives the same bytes as the one handed over, where only the band is set
    const vgx_planar_map_config defaults = PlanarMapConfig(cfg.z_min, cfg.z_max);
    if (defaults.min_free_voxels != 1 || defaults.use_box != 0 || defaults.max_distance_m != 2.0f) throw std::runtime_error("defaults");
    map.update(layer, cfg);
    wr(out, map, z);
    map.update(sm, VGX_EVAL_LAYER_TSDF, cfg);
    wr(out, map, z);
    map.update(sm, VGX_EVAL_LAYER_ESDF, cfg);
    wr(out, map, z);
    bool refused = false;  // an unset band throws
    try {
      vgx_planar_map_config unset;
      vgx_planar_map_config_default(&unset);
      map.update(layer, unset);
    } catch (const std::runtime_error&) {
      refused = true;
    }
    if (!refused) throw std::runtime_error("an unset band was served");
  } catch (const std::exception& e) {
    std::printf("FAILED %s\n", e.what());
    return 6;
  }
  fclose(out);
  vgx_tsdf_layer_destroy(layer);
  vgx_submap_destroy(sm);
  vgx_ctx_destroy(ctx);
  std::printf("PLANAR_MAP_SMOKE_OK\n");
  return 0;
}
