// GetProjectedMapOnGpu (voxgraph_amd/cpp/gpu_projected_map.h) from plain C++ against the stand-in cblox / voxblox
// headers: reads submaps (ID, pose, TSDF blocks) from argv[1], fills a cblox::SubmapCollection in FILE order, projects
// it on the GPU, hands the layer to a voxblox::Layer through DownloadTsdfLayer and writes that layer's blocks (sorted)
// to argv[2].  tests/test_projected_map_cpp.py compares the result with the Python path.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include <cblox/core/submap_collection.h>
#include <cblox/core/tsdf_esdf_submap.h>

#include "gpu_projected_map.h"
#include "gpu_tsdf_layer_bridge.h"

// the two things GpuSubmapRegistry reads beyond cblox's submap: registration-point sets (empty here)
class ProjSubmap : public cblox::TsdfEsdfSubmap {
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

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t n = 0, vps = 0;
  float vs = 0;
  get(in, &n, 1);
  get(in, &vps, 1);
  get(in, &vs, 1);
  const size_t vox = static_cast<size_t>(vps) * vps * vps;
  cblox::SubmapCollection<ProjSubmap> collection;
  for (int32_t s = 0; s < n; ++s) {
    int32_t id = 0, nb = 0;
    float T[7];
    get(in, &id, 1);
    get(in, &nb, 1);
    get(in, T, 7);
    std::vector<int32_t> bi(3 * static_cast<size_t>(nb));
    std::vector<float> d(vox * nb), w(vox * nb);
    get(in, bi.data(), bi.size());
    get(in, d.data(), d.size());
    get(in, w.data(), w.size());
    ProjSubmap::Config cfg;
    cfg.tsdf_voxel_size = vs;
    cfg.tsdf_voxels_per_side = static_cast<size_t>(vps);
    cfg.esdf_voxel_size = vs;
    cfg.esdf_voxels_per_side = static_cast<size_t>(vps);
    const voxblox::Transformation pose(voxblox::Transformation::Rotation(T[0], T[1], T[2], T[3]),
                                       voxblox::Transformation::Position(T[4], T[5], T[6]));
    auto sm = std::make_shared<ProjSubmap>(pose, static_cast<cblox::SubmapID>(id), cfg);
    voxblox::Layer<voxblox::TsdfVoxel>* layer = sm->getTsdfMapPtr()->getTsdfLayerPtr();
    for (int32_t b = 0; b < nb; ++b) {
      voxblox::BlockIndex idx;
      idx[0] = bi[3 * b];
      idx[1] = bi[3 * b + 1];
      idx[2] = bi[3 * b + 2];
      auto block = layer->allocateBlockPtrByIndex(idx);
      for (size_t i = 0; i < vox; ++i) {
        block->getVoxelByLinearIndex(i).distance = d[b * vox + i];
        block->getVoxelByLinearIndex(i).weight = w[b * vox + i];
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
    voxgraph_amd::GpuSubmapRegistry::instance().setContext(ctx);
    voxgraph_amd::GpuTsdfLayer gpu_layer(ctx, vs, vps);
    voxgraph_amd::GetProjectedMapOnGpu(collection, &gpu_layer);
    voxblox::Layer<voxblox::TsdfVoxel> projected(vs, static_cast<size_t>(vps));
    voxgraph_amd::DownloadTsdfLayer(gpu_layer, &projected);
    voxblox::BlockIndexList blocks;
    projected.getAllAllocatedBlocks(&blocks);
    std::sort(blocks.begin(), blocks.end(), [](const voxblox::BlockIndex& a, const voxblox::BlockIndex& b) {
      return a[0] != b[0] ? a[0] < b[0] : (a[1] != b[1] ? a[1] < b[1] : a[2] < b[2]);
    });
    std::ofstream out(argv[2], std::ios::binary);
    const int32_t nb = static_cast<int32_t>(blocks.size());
    out.write(reinterpret_cast<const char*>(&nb), 4);
    for (const auto& idx : blocks) {
      const int32_t i3[3] = {idx[0], idx[1], idx[2]};
      out.write(reinterpret_cast<const char*>(i3), 12);
      const auto& block = projected.getBlockByIndex(idx);
      for (size_t i = 0; i < vox; ++i) out.write(reinterpret_cast<const char*>(&block.getVoxelByLinearIndex(i).distance), 4);
      for (size_t i = 0; i < vox; ++i) out.write(reinterpret_cast<const char*>(&block.getVoxelByLinearIndex(i).weight), 4);
    }
    rc = out ? 0 : 4;
    voxgraph_amd::GpuSubmapRegistry::instance().clear();
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("PROJECTED_MAP_SMOKE_OK\n");
  return rc;
}
