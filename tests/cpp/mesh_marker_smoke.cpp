// voxgraph's three mesh markers (voxgraph_amd/cpp/gpu_mesh_marker.h) from plain C++ against the stand-in cblox / voxblox
// headers and the stand-in visualization_msgs/Marker (marker_standin.h).
//   mesh_marker_smoke compile     no device: the header instantiates on the stand-ins, the mode and type values
//   mesh_marker_smoke IN OUT      IN: submaps (ID, pose, TSDF blocks) in the layout of separated_mesh_smoke.cpp
//                                 OUT: three markers -- the combined mesh (kNormals, opacity 0.5), the separated mesh
//                                 (kLambertColor, 0.75) and the mesh of the submap with the smallest ID in voxgraph's colour
//                                 of it (opacity 1) -- each as its fixed fields, then points and colors
// tests/test_mesh_marker_cpp.py compares them with the restatement (tests/mesh_marker_ref.py) over the Python path's meshes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include <cblox/core/submap_collection.h>
#include <cblox/core/tsdf_esdf_submap.h>

#include "gpu_mesh_marker.h"
#include "marker_standin.h"

// the two things GpuSubmapRegistry reads beyond cblox's submap: registration-point sets (empty here)
class MarkerSubmap : public cblox::TsdfEsdfSubmap {
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

using Collection = cblox::SubmapCollection<MarkerSubmap>;
using voxgraph_amd::MarkerColorMode;

template <typename T>
static void get(std::ifstream& in, T* p, size_t n) {
  in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
  if (!in) throw std::runtime_error("short input file");
}

template <typename T>
static void put(std::ofstream& out, const T* p, size_t n) {
  out.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(n * sizeof(T)));
}

static int compile_checks() {
  if (static_cast<int>(MarkerColorMode::kColor) != 0 || static_cast<int>(MarkerColorMode::kHeight) != 1 ||
      static_cast<int>(MarkerColorMode::kNormals) != 2 || static_cast<int>(MarkerColorMode::kGray) != 3 ||
      static_cast<int>(MarkerColorMode::kLambert) != 4 || static_cast<int>(MarkerColorMode::kLambertColor) != 5)
    return 10;
  if (voxgraph_amd::kMarkerTriangleList != standin_marker::Marker::TRIANGLE_LIST) return 11;
  vgx_mesh_marker_config cfg;
  vgx_mesh_marker_config_default(&cfg);
  if (cfg.color_mode != VGX_MARKER_LAMBERT_COLOR || cfg.opacity != 1.0f || cfg.use_constant_color != 0) return 12;
  // the templates instantiate on the stand-ins (taken by address: nothing runs without a device)
  auto f1 = &voxgraph_amd::CombinedMeshMarkerOnGpu<Collection>;
  auto f2 = &voxgraph_amd::SeparatedMeshMarkerOnGpu<Collection>;
  auto f3 = &voxgraph_amd::DownloadMarker<standin_marker::Marker>;
  auto f4 = &voxgraph_amd::ColoredMeshMarkerOnGpu;
  if (!f1 || !f2 || !f3 || !f4) return 13;
  std::printf("MESH_MARKER_COMPILE_OK\n");
  return 0;
}

// the fixed fields, then the arrays; 0 when the header was left alone
static int write_marker(std::ofstream& out, const standin_marker::Marker& m) {
  if (m.header.frame_id != "mission" || m.header.stamp != 12.5 || m.id != 42) return 20;
  if (m.points.size() != m.colors.size()) return 21;
  const int64_t n = static_cast<int64_t>(m.points.size());
  const int32_t head[3] = {m.type, static_cast<int32_t>(m.frame_locked), static_cast<int32_t>(m.ns.size())};
  const double nums[7] = {m.scale.x, m.scale.y, m.scale.z, m.pose.orientation.x, m.pose.orientation.y, m.pose.orientation.z,
                          m.pose.orientation.w};
  put(out, &n, 1);
  put(out, head, 3);
  put(out, m.ns.data(), m.ns.size());
  put(out, nums, 7);
  put(out, &m.color.a, 1);
  put(out, reinterpret_cast<const double*>(m.points.data()), 3 * m.points.size());
  put(out, reinterpret_cast<const float*>(m.colors.data()), 4 * m.colors.size());
  return out ? 0 : 22;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "compile") == 0) return compile_checks();
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  int32_t n = 0, vps = 0;
  float vs = 0, min_weight = 0;
  get(in, &n, 1);
  get(in, &vps, 1);
  get(in, &vs, 1);
  get(in, &min_weight, 1);
  const size_t vox = static_cast<size_t>(vps) * vps * vps;
  Collection collection;
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
    MarkerSubmap::Config cfg;
    cfg.tsdf_voxel_size = vs;
    cfg.tsdf_voxels_per_side = static_cast<size_t>(vps);
    cfg.esdf_voxel_size = vs;
    cfg.esdf_voxels_per_side = static_cast<size_t>(vps);
    const voxblox::Transformation pose(voxblox::Transformation::Rotation(T[0], T[1], T[2], T[3]),
                                       voxblox::Transformation::Position(T[4], T[5], T[6]));
    auto sm = std::make_shared<MarkerSubmap>(pose, static_cast<cblox::SubmapID>(id), cfg);
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
    voxgraph_amd::GpuSubmapRegistry& registry = voxgraph_amd::GpuSubmapRegistry::instance();
    registry.setContext(ctx);
    voxgraph_amd::GpuTsdfLayer gpu_layer(ctx, vs, vps);
    voxgraph_amd::GpuMesh gpu_mesh(ctx);
    voxgraph_amd::GpuMeshMarker gpu_marker(ctx);
    std::ofstream out(argv[2], std::ios::binary);
    for (int pass = 0; pass < 3 && rc == 0; ++pass) {
      standin_marker::Marker marker;  // the header and the id are the caller's
      marker.header.frame_id = "mission";
      marker.header.stamp = 12.5;
      marker.id = 42;
      if (pass == 0) {
        voxgraph_amd::CombinedMeshMarkerOnGpu(collection, &gpu_layer, min_weight, 0.5f, &gpu_mesh, &gpu_marker);
      } else if (pass == 1) {
        voxgraph_amd::SeparatedMeshMarkerOnGpu(collection, min_weight, 0.75f, &gpu_mesh, &gpu_marker);
      } else {
        const auto id = collection.getIDs().front();  // ascending IDs: the smallest
        vgx_mesh_config cfg;
        vgx_mesh_config_default(&cfg);
        cfg.min_weight = min_weight;
        if (vgx_submap_generate_mesh(registry.handleOf(collection.getSubmapConstPtr(id)), &cfg, gpu_mesh.handle()) != VGX_OK) {
          rc = 5;
          break;
        }
        voxgraph_amd::ColoredMeshMarkerOnGpu(gpu_mesh, voxgraph_amd::SubmapColor(static_cast<int>(id)), 1.0f, &gpu_marker);
      }
      voxgraph_amd::DownloadMarker(gpu_marker, &marker);
      rc = write_marker(out, marker);
    }
    registry.clear();
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("MESH_MARKER_SMOKE_OK\n");
  return rc;
}
