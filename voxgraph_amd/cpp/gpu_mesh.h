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
// Semantics and deviations (no colour, no incremental meshing) are stated at vgx_tsdf_layer_generate_mesh in
// include/voxgraph_amd.h.
#ifndef VOXGRAPH_AMD_CPP_GPU_MESH_H_
#define VOXGRAPH_AMD_CPP_GPU_MESH_H_

#include <voxblox/core/common.h>

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

 private:
  void check(int rc, const char* what) const {
    if (rc != VGX_OK) throw std::runtime_error(std::string(what) + ": " + vgx_last_error(ctx_));
  }
  vgx_ctx ctx_;
  vgx_mesh mesh_ = nullptr;
};

// MeshIntegrator<TsdfVoxel>::generateMesh(false, false) over a layer on the GPU (queued behind its scans / merges)
inline GpuMesh& GenerateMeshOnGpu(const GpuTsdfLayer& layer, float min_weight, GpuMesh* mesh) {
  if (!mesh) throw std::invalid_argument("GenerateMeshOnGpu: mesh == nullptr");
  vgx_mesh_config cfg;
  vgx_mesh_config_default(&cfg);
  cfg.min_weight = min_weight;
  if (vgx_tsdf_layer_generate_mesh(layer.handle(), &cfg, mesh->handle()) != VGX_OK)
    throw std::runtime_error(std::string("vgx_tsdf_layer_generate_mesh: ") + layer.last_error());
  return *mesh;
}

// cblox SubmapMesher::generateCombinedMesh: the projected map of the collection (submaps in ID order, at their poses)
// into gpu_layer, then its mesh
template <typename CollectionT>
GpuMesh& GenerateCombinedMeshOnGpu(const CollectionT& collection, GpuTsdfLayer* gpu_layer, float min_weight, GpuMesh* mesh) {
  GetProjectedMapOnGpu(collection, gpu_layer);
  return GenerateMeshOnGpu(*gpu_layer, min_weight, mesh);
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

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_MESH_H_
