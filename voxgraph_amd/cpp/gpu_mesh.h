// The combined mesh on the GPU: cblox SubmapMesher::generateCombinedMesh and voxblox MeshIntegrator<TsdfVoxel>.
//
// voxgraph meshes its map after every optimisation (VoxgraphMapper::publishMaps -> SubmapVisuals::publishCombinedMesh on
// a background thread) and on request (saveCombinedMesh): the projected map, then MeshIntegrator::generateMesh(false,
// false) on it.  With the projected map already on the GPU (gpu_projected_map.h) the mesh is made there too:
//
//   voxgraph_amd::GpuTsdfLayer gpu_layer(ctx, voxel_size, voxels_per_side);
//   voxgraph_amd::GpuMesh gpu_mesh(ctx);                                          (kept: its buffers are reused)
//   voxgraph_amd::GenerateCombinedMeshOnGpu(submap_collection, &gpu_layer, mesh_config.min_weight, &gpu_mesh);
//   voxblox::MeshLayer mesh_layer(submap_collection.block_size());
//   voxgraph_amd::DownloadMeshLayer(gpu_mesh, &mesh_layer);
//
// Semantics and deviations (no incremental meshing) are stated at vgx_tsdf_layer_generate_mesh in include/voxgraph_amd.h.
// MeshIntegratorConfig::use_color is an opt-in, off by default (the last argument of GenerateMeshOnGpu /
// GenerateCombinedMeshOnGpu): one TSDF colour per vertex, which DownloadColoredMeshLayer, writePly, the weld and the
// markers then carry -- more than zeros only when the submaps kept their colours (GpuSubmapRegistry::setKeepColors).
//
// The separated mesh (SubmapVisuals::publishSeparatedMesh / saveSeparatedMesh: cblox generateSeparatedMesh) is one call
// over the whole collection, each submap in voxgraph's colour (vgx_submaps_generate_separated_mesh):
//
//   voxgraph_amd::GenerateSeparatedMeshOnGpu(submap_collection, mesh_config.min_weight, &gpu_mesh);
//   voxgraph_amd::DownloadColoredMeshLayer(gpu_mesh, &mesh_layer);
//
// The connected mesh (what saveCombinedMesh / saveSeparatedMesh write through voxblox::outputMeshLayerAsPly, and
// MeshLayer::getConnectedMesh returns): the soup's vertices welded on the GPU, an index list (vgx_mesh_connect):
//
//   voxgraph_amd::GpuConnectedMesh gpu_connected(ctx);                            (kept: its buffers are reused)
//   voxgraph_amd::ConnectMeshOnGpu(gpu_mesh, 1e-10f, &gpu_connected);
//   gpu_connected.writePly(filepath);              or   voxblox::Mesh mesh; DownloadConnectedMesh(gpu_connected, &mesh);
#ifndef VOXGRAPH_AMD_CPP_GPU_MESH_H_
#define VOXGRAPH_AMD_CPP_GPU_MESH_H_

#include <voxblox/core/common.h>

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_fast_tsdf_integrator.h"
#include "gpu_projected_map.h"

namespace voxgraph_amd {

// A mesh on the GPU (vgx_mesh): per allocated TSDF block, in ascending block-index order, a range of triangles.
class GpuMesh {
 public:
  explicit GpuMesh(vgx_ctx ctx) : ctx_(ctx) {
    if (vgx_mesh_create(ctx, &mesh_) != VGX_OK) throw std::runtime_error(std::string("vgx_mesh_create: ") + vgx_last_error(ctx));
  }
  ~GpuMesh() { vgx_mesh_destroy(mesh_); }
  GpuMesh(const GpuMesh&) = delete;
  GpuMesh& operator=(const GpuMesh&) = delete;
  vgx_mesh handle() const { return mesh_; }
  const char* last_error() const { return vgx_last_error(ctx_); }
  void stats(int32_t* n_blocks, int64_t* n_triangles) const { check(vgx_mesh_stats(mesh_, n_blocks, n_triangles), "vgx_mesh_stats"); }
  // block_index [nb][3], first [nb+1], vertices [T][3][3], normals [T][3]
  void download(std::vector<int32_t>* block_index, std::vector<int64_t>* first, std::vector<float>* vertices,
                std::vector<float>* normals) const {
    int32_t nb = 0;
    int64_t nt = 0;
    stats(&nb, &nt);
    block_index->resize(3 * static_cast<size_t>(nb));
    first->resize(static_cast<size_t>(nb) + 1);
    vertices->resize(9 * static_cast<size_t>(nt));
    normals->resize(3 * static_cast<size_t>(nt));
    check(vgx_mesh_download(mesh_, block_index->data(), first->data(), vertices->data(), normals->data()), "vgx_mesh_download");
  }
  void writePly(const std::string& path) const { check(vgx_mesh_write_ply(mesh_, path.c_str()), "vgx_mesh_write_ply"); }
  bool hasColors() const {
    int32_t has = 0;
    check(vgx_mesh_has_colors(mesh_, &has), "vgx_mesh_has_colors");
    return has != 0;
  }
  // VGX_MESH_COLORS_NONE / _PER_TRIANGLE (a separated mesh) / _PER_VERTEX (a use_color mesh)
  int32_t colorLayout() const {
    int32_t layout = 0;
    check(vgx_mesh_color_layout(mesh_, &layout), "vgx_mesh_color_layout");
    return layout;
  }
  // rgba [T][4], one colour per triangle (a separated mesh; throws on any other mesh)
  void downloadColors(std::vector<uint8_t>* rgba) const {
    int32_t nb = 0;
    int64_t nt = 0;
    stats(&nb, &nt);
    rgba->resize(4 * static_cast<size_t>(nt));
    check(vgx_mesh_download_colors(mesh_, rgba->data()), "vgx_mesh_download_colors");
  }
  // rgba [T][3][4], one colour per soup vertex (a use_color mesh; throws on any other mesh)
  void downloadVertexColors(std::vector<uint8_t>* rgba) const {
    int32_t nb = 0;
    int64_t nt = 0;
    stats(&nb, &nt);
    rgba->resize(12 * static_cast<size_t>(nt));
    check(vgx_mesh_download_vertex_colors(mesh_, rgba->data()), "vgx_mesh_download_vertex_colors");
  }

 private:
  void check(int rc, const char* what) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string(what) + ": " + vgx_last_error(ctx_));
  }
  vgx_ctx ctx_;
  vgx_mesh mesh_ = nullptr;
};

// MeshIntegrator<TsdfVoxel>::generateMesh(false, false) over a layer on the GPU (queued behind its scans / merges).
// use_color (MeshIntegratorConfig::use_color; off by default): one TSDF colour per vertex as well
inline GpuMesh& GenerateMeshOnGpu(const GpuTsdfLayer& layer, float min_weight, GpuMesh* mesh, bool use_color = false) {
  if (!mesh) throw std::invalid_argument("GenerateMeshOnGpu: mesh == nullptr");
  vgx_mesh_config cfg;
  vgx_mesh_config_default(&cfg);
  cfg.min_weight = min_weight;
  const int rc = use_color ? vgx_tsdf_layer_generate_mesh_colored(layer.handle(), &cfg, mesh->handle())
                           : vgx_tsdf_layer_generate_mesh(layer.handle(), &cfg, mesh->handle());
  if (rc != VGX_OK)
    throw std::runtime_error(std::string(use_color ? "vgx_tsdf_layer_generate_mesh_colored: " : "vgx_tsdf_layer_generate_mesh: ") +
                             layer.last_error());
  return *mesh;
}

// cblox SubmapMesher::generateCombinedMesh: the projected map of the collection (submaps in ID order, at their poses)
// into gpu_layer, then its mesh
template <typename CollectionT>
GpuMesh& GenerateCombinedMeshOnGpu(const CollectionT& collection, GpuTsdfLayer* gpu_layer, float min_weight, GpuMesh* mesh,
                                   bool use_color = false) {
  GetProjectedMapOnGpu(collection, gpu_layer);
  return GenerateMeshOnGpu(*gpu_layer, min_weight, mesh, use_color);
}

// voxblox rainbowColorMap [recalled]: an HSV blend at s = v = 1 in double, channels truncated to uint8, a = 255
inline voxblox::Color RainbowColorMap(double h) {
  h -= std::floor(h);
  h *= 6.0;
  const int i = static_cast<int>(std::floor(h));
  double f = h - i;
  if (!(i & 1)) f = 1.0 - f;
  const double v = 1.0, m = 0.0, n = 1.0 - f;
  double r = 255, g = 127, b = 127;
  switch (i) {
    case 6:
    case 0: r = 255 * v; g = 255 * n; b = 255 * m; break;
    case 1: r = 255 * n; g = 255 * v; b = 255 * m; break;
    case 2: r = 255 * m; g = 255 * v; b = 255 * n; break;
    case 3: r = 255 * m; g = 255 * n; b = 255 * v; break;
    case 4: r = 255 * n; g = 255 * m; b = 255 * v; break;
    case 5: r = 255 * v; g = 255 * m; b = 255 * n; break;
    default: break;
  }
  return voxblox::Color(static_cast<uint8_t>(r), static_cast<uint8_t>(g), static_cast<uint8_t>(b), 255);
}

constexpr int kDefaultColorCycleLength = 20;  // cblox::kDefaultColorCycleLength [recalled]

// voxgraph's colour of a submap's mesh (VoxgraphMapper::publishActiveSubmapMeshCallback)
inline voxblox::Color SubmapColor(int submap_id) {
  return RainbowColorMap(static_cast<double>(submap_id) / static_cast<double>(kDefaultColorCycleLength));
}

// cblox SubmapMesher::generateSeparatedMesh: the collection's submaps in ascending ID order at getPose(), submap ID
// coloured colors[k] (k its rank in that order), meshed in one call (vgx_submaps_generate_separated_mesh)
template <typename CollectionT>
GpuMesh& GenerateSeparatedMeshOnGpu(const CollectionT& collection, const std::vector<voxblox::Color>& colors, float min_weight,
                                    GpuMesh* mesh) {
  if (!mesh) throw std::invalid_argument("GenerateSeparatedMeshOnGpu: mesh == nullptr");
  GpuSubmapRegistry& registry = GpuSubmapRegistry::instance();
  std::vector<vgx_submap> handles;
  std::vector<float> T_M_S;
  std::vector<uint8_t> rgba;
  for (const auto id : collection.getIDs()) {  // cblox keeps its submaps in a std::map: ascending IDs
    const auto submap_ptr = collection.getSubmapConstPtr(id);
    handles.push_back(registry.handleOf(submap_ptr));
    const auto& pose = submap_ptr->getPose();
    const auto& q = pose.getRotation();
    const auto& t = pose.getPosition();
    const float T[7] = {static_cast<float>(q.w()), static_cast<float>(q.x()), static_cast<float>(q.y()),
                        static_cast<float>(q.z()), static_cast<float>(t[0]),  static_cast<float>(t[1]),
                        static_cast<float>(t[2])};
    T_M_S.insert(T_M_S.end(), T, T + 7);
  }
  if (colors.size() != handles.size()) throw std::invalid_argument("GenerateSeparatedMeshOnGpu: one colour per submap");
  for (const voxblox::Color& c : colors) {
    rgba.push_back(c.r);
    rgba.push_back(c.g);
    rgba.push_back(c.b);
    rgba.push_back(c.a);
  }
  vgx_mesh_config cfg;
  vgx_mesh_config_default(&cfg);
  cfg.min_weight = min_weight;
  if (vgx_submaps_generate_separated_mesh(registry.context(), static_cast<int32_t>(handles.size()), handles.data(),
                                          T_M_S.data(), rgba.data(), &cfg, mesh->handle()) != VGX_OK)
    throw std::runtime_error(std::string("vgx_submaps_generate_separated_mesh: ") + mesh->last_error());
  return *mesh;
}

// ... with voxgraph's colours (SubmapColor of each ID)
template <typename CollectionT>
GpuMesh& GenerateSeparatedMeshOnGpu(const CollectionT& collection, float min_weight, GpuMesh* mesh) {
  std::vector<voxblox::Color> colors;
  for (const auto id : collection.getIDs()) colors.push_back(SubmapColor(static_cast<int>(id)));
  return GenerateSeparatedMeshOnGpu(collection, colors, min_weight, mesh);
}

// Fills a voxblox-shaped MeshLayer (allocateMeshPtrByIndex(BlockIndex) returning a mesh pointer with vertices, normals
// and indices): one mesh per allocated TSDF block, possibly empty, each holding its triangle soup -- three vertices per
// triangle, the triangle's normal on each, indices 0..3n-1.  No colours (the GPU mesh has none).
template <typename MeshLayerT>
void DownloadMeshLayer(const GpuMesh& gpu_mesh, MeshLayerT* mesh_layer) {
  if (!mesh_layer) throw std::invalid_argument("DownloadMeshLayer: mesh_layer == nullptr");
  std::vector<int32_t> bi;
  std::vector<int64_t> first;
  std::vector<float> v, n;
  gpu_mesh.download(&bi, &first, &v, &n);
  for (size_t b = 0; b + 1 < first.size(); ++b) {
    voxblox::BlockIndex index;
    index[0] = bi[3 * b];
    index[1] = bi[3 * b + 1];
    index[2] = bi[3 * b + 2];
    auto mesh = mesh_layer->allocateMeshPtrByIndex(index);
    mesh->vertices.clear();
    mesh->normals.clear();
    mesh->indices.clear();
    for (int64_t t = first[b]; t < first[b + 1]; ++t) {
      const voxblox::Point normal(n[3 * t], n[3 * t + 1], n[3 * t + 2]);
      for (int q = 0; q < 3; ++q) {
        const float* p = &v[9 * t + 3 * q];
        mesh->indices.push_back(static_cast<int>(mesh->vertices.size()));
        mesh->vertices.push_back(voxblox::Point(p[0], p[1], p[2]));
        mesh->normals.push_back(normal);
      }
    }
  }
}

// DownloadMeshLayer plus the colours: mesh->colors gets, on each vertex, the triangle's colour (a separated mesh) or the
// vertex's own (a use_color mesh) -- voxblox's layout either way.  The MeshLayer's mesh type needs a `colors` vector of
// voxblox::Color.
template <typename MeshLayerT>
void DownloadColoredMeshLayer(const GpuMesh& gpu_mesh, MeshLayerT* mesh_layer) {
  if (!mesh_layer) throw std::invalid_argument("DownloadColoredMeshLayer: mesh_layer == nullptr");
  std::vector<int32_t> bi;
  std::vector<int64_t> first;
  std::vector<float> v, n;
  std::vector<uint8_t> rgba;
  gpu_mesh.download(&bi, &first, &v, &n);
  const bool per_vertex = gpu_mesh.colorLayout() == VGX_MESH_COLORS_PER_VERTEX;
  if (per_vertex) gpu_mesh.downloadVertexColors(&rgba);
  else gpu_mesh.downloadColors(&rgba);
  for (size_t b = 0; b + 1 < first.size(); ++b) {
    voxblox::BlockIndex index;
    index[0] = bi[3 * b];
    index[1] = bi[3 * b + 1];
    index[2] = bi[3 * b + 2];
    auto mesh = mesh_layer->allocateMeshPtrByIndex(index);
    mesh->vertices.clear();
    mesh->normals.clear();
    mesh->colors.clear();
    mesh->indices.clear();
    for (int64_t t = first[b]; t < first[b + 1]; ++t) {
      const voxblox::Point normal(n[3 * t], n[3 * t + 1], n[3 * t + 2]);
      for (int q = 0; q < 3; ++q) {
        const uint8_t* c = &rgba[per_vertex ? 12 * t + 4 * q : 4 * t];
        const voxblox::Color color(c[0], c[1], c[2], c[3]);
        const float* p = &v[9 * t + 3 * q];
        mesh->indices.push_back(static_cast<int>(mesh->vertices.size()));
        mesh->vertices.push_back(voxblox::Point(p[0], p[1], p[2]));
        mesh->normals.push_back(normal);
        mesh->colors.push_back(color);
      }
    }
  }
}

// A connected mesh on the GPU (vgx_connected_mesh): unique vertices in order of first occurrence, [T][3] indices.
class GpuConnectedMesh {
 public:
  explicit GpuConnectedMesh(vgx_ctx ctx) : ctx_(ctx) {
    if (vgx_connected_mesh_create(ctx, &mesh_) != VGX_OK)
      throw std::runtime_error(std::string("vgx_connected_mesh_create: ") + vgx_last_error(ctx));
  }
  ~GpuConnectedMesh() { vgx_connected_mesh_destroy(mesh_); }
  GpuConnectedMesh(const GpuConnectedMesh&) = delete;
  GpuConnectedMesh& operator=(const GpuConnectedMesh&) = delete;
  vgx_connected_mesh handle() const { return mesh_; }
  const char* last_error() const { return vgx_last_error(ctx_); }
  void stats(int64_t* n_vertices, int64_t* n_triangles, bool* has_colors) const {
    int32_t has = 0;
    check(vgx_connected_mesh_stats(mesh_, n_vertices, n_triangles, &has), "vgx_connected_mesh_stats");
    if (has_colors) *has_colors = has != 0;
  }
  // vertices [V][3], normals [V][3], rgba [V][4] (left empty when the mesh has no colours), indices [T][3]
  void download(std::vector<float>* vertices, std::vector<float>* normals, std::vector<uint8_t>* rgba,
                std::vector<uint32_t>* indices) const {
    int64_t nv = 0, nt = 0;
    bool has = false;
    stats(&nv, &nt, &has);
    vertices->resize(3 * static_cast<size_t>(nv));
    normals->resize(3 * static_cast<size_t>(nv));
    rgba->resize(has ? 4 * static_cast<size_t>(nv) : 0);
    indices->resize(3 * static_cast<size_t>(nt));
    check(vgx_connected_mesh_download(mesh_, vertices->data(), normals->data(), has ? rgba->data() : nullptr, indices->data()),
          "vgx_connected_mesh_download");
  }
  void writePly(const std::string& path) const { check(vgx_connected_mesh_write_ply(mesh_, path.c_str()), "vgx_connected_mesh_write_ply"); }

 private:
  void check(int rc, const char* what) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string(what) + ": " + vgx_last_error(ctx_));
  }
  vgx_ctx ctx_;
  vgx_connected_mesh mesh_ = nullptr;
};

// MeshLayer::getConnectedMesh(&connected, approximate_vertex_proximity_threshold) over a mesh on the GPU
inline GpuConnectedMesh& ConnectMeshOnGpu(const GpuMesh& mesh, float approximate_vertex_proximity_threshold,
                                          GpuConnectedMesh* connected) {
  if (!connected) throw std::invalid_argument("ConnectMeshOnGpu: connected == nullptr");
  if (vgx_mesh_connect(mesh.handle(), approximate_vertex_proximity_threshold, connected->handle()) != VGX_OK)
    throw std::runtime_error(std::string("vgx_mesh_connect: ") + mesh.last_error());
  return *connected;
}

// Fills a voxblox-shaped Mesh (vertices, normals, colors, indices): the connected mesh as createConnectedMesh leaves it.
// colors stays empty when the GPU mesh has none.
template <typename MeshT>
void DownloadConnectedMesh(const GpuConnectedMesh& gpu_connected, MeshT* mesh) {
  if (!mesh) throw std::invalid_argument("DownloadConnectedMesh: mesh == nullptr");
  std::vector<float> v, n;
  std::vector<uint8_t> rgba;
  std::vector<uint32_t> idx;
  gpu_connected.download(&v, &n, &rgba, &idx);
  mesh->vertices.clear();
  mesh->normals.clear();
  mesh->colors.clear();
  mesh->indices.clear();
  for (size_t i = 0; 3 * i < v.size(); ++i) {
    mesh->vertices.push_back(voxblox::Point(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
    mesh->normals.push_back(voxblox::Point(n[3 * i], n[3 * i + 1], n[3 * i + 2]));
  }
  for (size_t i = 0; 4 * i < rgba.size(); ++i)
    mesh->colors.push_back(voxblox::Color(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]));
  mesh->indices.reserve(idx.size());
  for (const uint32_t i : idx) mesh->indices.push_back(i);
}

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_MESH_H_
