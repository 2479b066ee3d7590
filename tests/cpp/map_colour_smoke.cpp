// The colour opt-ins of the C++ mirrors from plain C++ against the stand-in cblox / voxblox headers:
// GpuSubmapRegistry::setKeepColors (UploadFinishedSubmap's keep_colors), GenerateCombinedMeshOnGpu's use_color,
// DownloadColoredMeshLayer and FillMarkerWithMeshOnGpu on the per-vertex mesh, FinishSubmapOnGpu's keep_colors.
// Reads submaps (ID, pose, TSDF blocks with colours) from argv[1], writes to argv[2]: the flags, the coloured MeshLayer in
// layer order, the kLambertColor marker colours.  tests/test_map_colour_cpp.py compares them with the Python path.
// `map_colour_smoke compile` touches no device: the defaults of the opt-ins.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include <cblox/core/submap_collection.h>
#include <cblox/core/tsdf_esdf_submap.h>

#include "gpu_mesh.h"
#include "gpu_mesh_marker.h"
#include "gpu_tsdf_layer_bridge.h"

// the parts of voxblox's Mesh / MeshLayer DownloadColoredMeshLayer fills
struct TestMesh {
  voxblox::AlignedVector<voxblox::Point> vertices;
  voxblox::AlignedVector<voxblox::Point> normals;
  std::vector<voxblox::Color> colors;
  std::vector<int> indices;
};
class TestMeshLayer {
 public:
  std::shared_ptr<TestMesh> allocateMeshPtrByIndex(const voxblox::BlockIndex& index) {
    blocks.push_back(index);
    meshes.push_back(std::make_shared<TestMesh>());
    return meshes.back();
  }
  std::vector<voxblox::BlockIndex> blocks;
  std::vector<std::shared_ptr<TestMesh>> meshes;
};

// the two things GpuSubmapRegistry reads beyond cblox's submap: registration-point sets (empty here)
class ColourSubmap : public cblox::TsdfEsdfSubmap {
 public:
  enum class RegistrationPointType { kIsosurfacePoints = 0, kVoxels = 1 };
  struct Point {
    voxblox::Point position;
    float distance = 0, weight = 0;
  };
  struct Sampler {
    size_t size() const { return 0; }
    const Point& operator[](int) const { return p; }
    Point p;
  };
  using cblox::TsdfEsdfSubmap::TsdfEsdfSubmap;
  const Sampler& getRegistrationPoints(RegistrationPointType) const { return sampler_; }

 private:
  Sampler sampler_;
};

template <typename T>
static void get(std::ifstream& in, T* p, size_t n) {
  in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input file");
}

// the opt-ins exist, with their defaults off: these calls name every defaulted argument's position
static void instantiate(const cblox::SubmapCollection<ColourSubmap>& collection, voxgraph_amd::GpuTsdfLayer* layer,
                        voxgraph_amd::GpuMesh* mesh, voxgraph_amd::GpuMeshMarker* marker, vgx_ctx ctx) {
  voxgraph_amd::GenerateCombinedMeshOnGpu(collection, layer, 1e-4f, mesh);
  voxgraph_amd::GenerateMeshOnGpu(*layer, 1e-4f, mesh);
  voxgraph_amd::CombinedMeshMarkerOnGpu(collection, layer, 1e-4f, 1.0f, mesh, marker);
  vgx_submap_destroy(voxgraph_amd::FinishSubmapOnGpu(ctx, *layer, 1));
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "compile") == 0) {
    void (*fn)(const cblox::SubmapCollection<ColourSubmap>&, voxgraph_amd::GpuTsdfLayer*, voxgraph_amd::GpuMesh*,
               voxgraph_amd::GpuMeshMarker*, vgx_ctx) = &instantiate;
    std::printf("MAP_COLOUR_COMPILE_OK %d %d %d %d\n", fn != nullptr, VGX_MESH_COLORS_NONE, VGX_MESH_COLORS_PER_TRIANGLE,
                VGX_MESH_COLORS_PER_VERTEX);
    return 0;
  }
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t n = 0, vps = 0;
  float vs = 0, min_weight = 0;
  get(in, &n, 1);
  get(in, &vps, 1);
  get(in, &vs, 1);
  get(in, &min_weight, 1);
  const size_t vox = static_cast<size_t>(vps) * vps * vps;
  cblox::SubmapCollection<ColourSubmap> collection;
  for (int32_t s = 0; s < n; ++s) {
    int32_t id = 0, nb = 0;
    float T[7];
    get(in, &id, 1);
    get(in, &nb, 1);
    get(in, T, 7);
    std::vector<int32_t> bi(3 * static_cast<size_t>(nb));
    std::vector<float> d(vox * nb), w(vox * nb);
    std::vector<uint8_t> c(4 * vox * nb);
    get(in, bi.data(), bi.size());
    get(in, d.data(), d.size());
    get(in, w.data(), w.size());
    get(in, c.data(), c.size());
    ColourSubmap::Config cfg;
    cfg.tsdf_voxel_size = vs;
    cfg.tsdf_voxels_per_side = static_cast<size_t>(vps);
    cfg.esdf_voxel_size = vs;
    cfg.esdf_voxels_per_side = static_cast<size_t>(vps);
    const voxblox::Transformation pose(voxblox::Transformation::Rotation(T[0], T[1], T[2], T[3]),
                                       voxblox::Transformation::Position(T[4], T[5], T[6]));
    auto sm = std::make_shared<ColourSubmap>(pose, static_cast<cblox::SubmapID>(id), cfg);
    voxblox::Layer<voxblox::TsdfVoxel>* layer = sm->getTsdfMapPtr()->getTsdfLayerPtr();
    for (int32_t b = 0; b < nb; ++b) {
      voxblox::BlockIndex idx;
      idx[0] = bi[3 * b];
      idx[1] = bi[3 * b + 1];
      idx[2] = bi[3 * b + 2];
      auto block = layer->allocateBlockPtrByIndex(idx);
      for (size_t i = 0; i < vox; ++i) {
        voxblox::TsdfVoxel& v = block->getVoxelByLinearIndex(i);
        v.distance = d[b * vox + i];
        v.weight = w[b * vox + i];
        const uint8_t* q = &c[4 * (b * vox + i)];
        v.color = voxblox::Color(q[0], q[1], q[2], q[3]);
      }
    }
    collection.addSubmap(sm);
  }
  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) {
    std::printf("no device: %s\n", vgx_last_error(nullptr));
    return 3;
  }
  int rc = 0;
  {
    auto& registry = voxgraph_amd::GpuSubmapRegistry::instance();
    registry.setContext(ctx);
    voxgraph_amd::GpuTsdfLayer gpu_layer(ctx, vs, vps);
    voxgraph_amd::GpuMesh gpu_mesh(ctx);
    voxgraph_amd::GpuMeshMarker gpu_marker(ctx);
    int32_t flags[6] = {0, 0, 0, 0, 0, 0};
    // the defaults: no submap keeps colours, the mesh has none
    voxgraph_amd::GenerateCombinedMeshOnGpu(collection, &gpu_layer, min_weight, &gpu_mesh);
    for (const auto id : collection.getIDs()) {
      int32_t has = 0;
      vgx_submap_has_colors(registry.handleOf(collection.getSubmapConstPtr(id)), &has);
      flags[0] += has;
    }
    flags[1] = gpu_mesh.colorLayout();
    registry.clear();
    // the opt-ins
    registry.setKeepColors(true);
    voxgraph_amd::CombinedMeshMarkerOnGpu(collection, &gpu_layer, min_weight, 0.7f, &gpu_mesh, &gpu_marker, true,
                                          voxgraph_amd::MarkerColorMode::kLambertColor);
    for (const auto id : collection.getIDs()) {
      int32_t has = 0;
      vgx_submap_has_colors(registry.handleOf(collection.getSubmapConstPtr(id)), &has);
      flags[2] += has;
    }
    flags[3] = gpu_mesh.colorLayout();
    vgx_submap plain = voxgraph_amd::FinishSubmapOnGpu(ctx, gpu_layer, 100);
    vgx_submap kept = voxgraph_amd::FinishSubmapOnGpu(ctx, gpu_layer, 101, true);
    vgx_submap_has_colors(plain, &flags[4]);
    vgx_submap_has_colors(kept, &flags[5]);
    const int32_t kept_blocks = vgx_submap_num_blocks(kept);
    std::vector<int32_t> kept_index(3 * static_cast<size_t>(kept_blocks));
    std::vector<uint8_t> kept_rgba(4 * vox * static_cast<size_t>(kept_blocks));
    vgx_submap_block_index(kept, kept_index.data());
    if (vgx_submap_download_colors(kept, kept_rgba.data()) != VGX_OK) rc = 5;
    vgx_submap_destroy(plain);
    vgx_submap_destroy(kept);
    TestMeshLayer mesh_layer;
    voxgraph_amd::DownloadColoredMeshLayer(gpu_mesh, &mesh_layer);
    int64_t n_points = 0;
    gpu_marker.stats(&n_points, nullptr);
    std::vector<float> marker_colors(4 * static_cast<size_t>(n_points));
    if (n_points > 0) gpu_marker.download(nullptr, marker_colors.data());
    std::ofstream out(argv[2], std::ios::binary);
    out.write(reinterpret_cast<const char*>(flags), sizeof(flags));
    const int32_t nb = static_cast<int32_t>(mesh_layer.blocks.size());
    out.write(reinterpret_cast<const char*>(&nb), 4);
    for (int32_t b = 0; b < nb; ++b) {
      const TestMesh& m = *mesh_layer.meshes[b];
      const int32_t head[4] = {mesh_layer.blocks[b][0], mesh_layer.blocks[b][1], mesh_layer.blocks[b][2],
                               static_cast<int32_t>(m.vertices.size())};
      out.write(reinterpret_cast<const char*>(head), 16);
      for (const auto& p : m.vertices) out.write(reinterpret_cast<const char*>(p.data()), 12);
      for (const auto& q : m.colors) {
        const uint8_t bytes[4] = {q.r, q.g, q.b, q.a};
        out.write(reinterpret_cast<const char*>(bytes), 4);
      }
    }
    out.write(reinterpret_cast<const char*>(&n_points), 8);
    out.write(reinterpret_cast<const char*>(marker_colors.data()), static_cast<std::streamsize>(4 * marker_colors.size()));
    out.write(reinterpret_cast<const char*>(&kept_blocks), 4);
    out.write(reinterpret_cast<const char*>(kept_index.data()), static_cast<std::streamsize>(4 * kept_index.size()));
    out.write(reinterpret_cast<const char*>(kept_rgba.data()), static_cast<std::streamsize>(kept_rgba.size()));
    if (rc == 0) rc = out ? 0 : 4;
    registry.setKeepColors(false);
    registry.clear();
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("MAP_COLOUR_SMOKE_OK\n");
  return rc;
}
