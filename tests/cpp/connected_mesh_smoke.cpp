// ConnectMeshOnGpu + DownloadConnectedMesh (voxgraph_amd/cpp/gpu_mesh.h) from plain C++ against the stand-in cblox /
// voxblox headers: reads submaps (ID, pose, TSDF blocks) and two thresholds from argv[1], fills a cblox::SubmapCollection
// in FILE order, makes its separated mesh (voxgraph's colours) and its combined mesh on the GPU, connects the first at
// threshold 0 and the second at threshold 1 into ONE reused GpuConnectedMesh, fills the minimal voxblox-shaped Mesh below
// and writes it to argv[2] and argv[3].  tests/test_connected_mesh_cpp.py compares them with the Python path
// (capi.Mesh.connect).
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include <cblox/core/submap_collection.h>
#include <cblox/core/tsdf_esdf_submap.h>

#include "gpu_mesh.h"

// the parts of voxblox's Mesh DownloadConnectedMesh fills
struct TestMesh {
  voxblox::AlignedVector<voxblox::Point> vertices;
  voxblox::AlignedVector<voxblox::Point> normals;
  std::vector<voxblox::Color> colors;
  std::vector<uint32_t> indices;
};

// the two things GpuSubmapRegistry reads beyond cblox's submap: registration-point sets (empty here)
class SepSubmap : public cblox::TsdfEsdfSubmap {
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
  if (argc != 4) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t n = 0, vps = 0;
  float vs = 0, min_weight = 0;
  get(in, &n, 1);
  get(in, &vps, 1);
  get(in, &vs, 1);
  get(in, &min_weight, 1);
  float threshold[2] = {0, 0};
  get(in, threshold, 2);
  const size_t vox = static_cast<size_t>(vps) * vps * vps;
  cblox::SubmapCollection<SepSubmap> collection;
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
    SepSubmap::Config cfg;
    cfg.tsdf_voxel_size = vs;
    cfg.tsdf_voxels_per_side = static_cast<size_t>(vps);
    cfg.esdf_voxel_size = vs;
    cfg.esdf_voxels_per_side = static_cast<size_t>(vps);
    const voxblox::Transformation pose(voxblox::Transformation::Rotation(T[0], T[1], T[2], T[3]),
                                       voxblox::Transformation::Position(T[4], T[5], T[6]));
    auto sm = std::make_shared<SepSubmap>(pose, static_cast<cblox::SubmapID>(id), cfg);
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
    voxgraph_amd::GpuMesh gpu_mesh(ctx);
    voxgraph_amd::GpuTsdfLayer gpu_layer(ctx, vs, vps);
    voxgraph_amd::GpuConnectedMesh gpu_connected(ctx);
    for (int pass = 0; pass < 2 && rc == 0; ++pass) {
      if (pass == 0)
        voxgraph_amd::GenerateSeparatedMeshOnGpu(collection, min_weight, &gpu_mesh);
      else
        voxgraph_amd::GenerateCombinedMeshOnGpu(collection, &gpu_layer, min_weight, &gpu_mesh);
      voxgraph_amd::ConnectMeshOnGpu(gpu_mesh, threshold[pass], &gpu_connected);
      int64_t nv = 0, nt = 0;
      bool has = false;
      gpu_connected.stats(&nv, &nt, &has);
      TestMesh m;
      m.colors.push_back(voxblox::Color(1, 2, 3, 4));  // (cleared by the download)
      voxgraph_amd::DownloadConnectedMesh(gpu_connected, &m);
      if (has != (pass == 0) || static_cast<int64_t>(m.vertices.size()) != nv || static_cast<int64_t>(m.indices.size()) != 3 * nt ||
          m.normals.size() != m.vertices.size() || m.colors.size() != (has ? m.vertices.size() : 0)) {
        rc = 5;
        break;
      }
      std::ofstream out(argv[2 + pass], std::ios::binary);
      const int64_t head[3] = {nv, nt, has ? 1 : 0};
      out.write(reinterpret_cast<const char*>(head), 24);
      for (const auto& p : m.vertices) out.write(reinterpret_cast<const char*>(p.data()), 12);
      for (const auto& p : m.normals) out.write(reinterpret_cast<const char*>(p.data()), 12);
      for (const auto& c : m.colors) {
        const uint8_t rgba[4] = {c.r, c.g, c.b, c.a};
        out.write(reinterpret_cast<const char*>(rgba), 4);
      }
      out.write(reinterpret_cast<const char*>(m.indices.data()), static_cast<std::streamsize>(4 * m.indices.size()));
      rc = out ? 0 : 4;
    }
    voxgraph_amd::GpuSubmapRegistry::instance().clear();
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("CONNECTED_MESH_SMOKE_OK\n");
  return rc;
}
