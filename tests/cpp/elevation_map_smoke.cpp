// The elevation map (voxgraph_amd/cpp/gpu_elevation_map.h) from plain C++: a GridMap stand-in of a vgx_tsdf_layer and of a
// finished submap's two layers, written for tests/test_elevation_map_cpp.py to compare with the Python path.
//   elevation_map_smoke IN OUT
// IN: int32 vps, n_blocks; f32 voxel_size; the vgx_elevation_map_config (bytes); int32 block_index [nb][3]; f32 tsdf_d,
//     tsdf_w, esdf_d [nb][vps^3]; u8 esdf_o [nb][vps^3]
// OUT, per source (layer, submap TSDF, submap ESDF): f64 resolution, length_x, length_y, centre x, y, z; u32 H, W (from the
//     layout); int64 state counts [4], class counts [3]; then the six layers, f32 [H][W] each, in the message's order
#include <cstdio>
#include <vector>

#include "gpu_elevation_map.h"
#include "grid_map_standin.h"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}
void wr(FILE* out, const voxgraph_amd::GpuElevationMap& map, double z) {
  grid_map_msgs_standin::GridMap grid;
  map.toGridMap(&grid, z);
  static const char* const kLayers[6] = {"elevation", "slope", "step", "headroom", "traversability", "distance"};
  if (grid.layers.size() != 6 || grid.data.size() != 6 || grid.basic_layers != std::vector<std::string>{"elevation"})
    throw std::runtime_error("layers");
  for (int k = 0; k < 6; ++k)
    if (grid.layers[k] != kLayers[k]) throw std::runtime_error("layer names");
  int64_t states[4], classes[3];
  map.counts(states, classes);
  const uint32_t h = grid.data[0].layout.dim[0].size, w = grid.data[0].layout.dim[1].size;
  if ((int32_t)w != map.width() || (int32_t)h != map.height()) throw std::runtime_error("layout");
  const double info[6] = {grid.info.resolution,      grid.info.length_x,        grid.info.length_y,
                          grid.info.pose.position.x, grid.info.pose.position.y, grid.info.pose.position.z};
  fwrite(info, 8, 6, out);
  fwrite(&h, 4, 1, out);
  fwrite(&w, 4, 1, out);
  fwrite(states, 8, 4, out);
  fwrite(classes, 8, 3, out);
  for (const auto& layer : grid.data) {
    if (layer.data.size() != (size_t)w * h) throw std::runtime_error("layer size");
    fwrite(layer.data.data(), 4, layer.data.size(), out);
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t vps = 0, nb = 0;
  float vs = 0;
  vgx_elevation_map_config cfg;
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
    GpuElevationMap map(ctx);  // one handle, reused
    // a config built the C++ way carries the defaults, where only the band is set
    const vgx_elevation_map_config defaults = ElevationMapConfig(cfg.z_min, cfg.z_max);
    if (defaults.min_free_voxels != 1 || defaults.step_radius_cells != 1 || defaults.max_slope != 1.0f || defaults.max_step_m != 0.2f ||
        defaults.hole_is_obstacle != 1 || defaults.use_box != 0 || defaults.max_distance_m != 2.0f)
      throw std::runtime_error("defaults");
    map.update(layer, cfg);
    wr(out, map, z);
    map.update(sm, VGX_EVAL_LAYER_TSDF, cfg);
    wr(out, map, z);
    map.update(sm, VGX_EVAL_LAYER_ESDF, cfg);
    wr(out, map, z);
    bool refused = false;  // an unset band throws
    try {
      vgx_elevation_map_config unset;
      vgx_elevation_map_config_default(&unset);
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
  std::printf("ELEVATION_MAP_SMOKE_OK\n");
  return 0;
}
