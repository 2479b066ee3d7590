// GpuMapEvaluation::evaluate (voxgraph_amd/cpp/gpu_map_evaluation.h) from plain C++ against the stand-in cblox / voxblox
// headers and the Ceres stand-in of tests/stubs: reads submaps (ID, pose, TSDF blocks) and a ground-truth TSDF layer from
// argv[1], fills a cblox::SubmapCollection, evaluates the map on the GPU and prints the aligned pose, the solver's
// iterations, T_ground_truth__reading and the details (floats as hex, exactly).  tests/test_map_eval_cpp.py compares
// them with the Python path.
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include <cblox/core/submap_collection.h>
#include <cblox/core/tsdf_esdf_submap.h>

#include "gpu_map_evaluation.h"

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

static void read_blocks(std::ifstream& in, size_t vox, int32_t nb, std::vector<int32_t>* bi, std::vector<float>* d,
                        std::vector<float>* w) {
  bi->resize(3 * static_cast<size_t>(nb));
  d->resize(vox * nb);
  w->resize(vox * nb);
  get(in, bi->data(), bi->size());
  get(in, d->data(), d->size());
  get(in, w->data(), w->size());
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
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
    std::vector<int32_t> bi;
    std::vector<float> d, w;
    read_blocks(in, vox, nb, &bi, &d, &w);
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
  int32_t gt_nb = 0;
  get(in, &gt_nb, 1);
  std::vector<int32_t> gt_bi;
  std::vector<float> gt_d, gt_w;
  read_blocks(in, vox, gt_nb, &gt_bi, &gt_d, &gt_w);
  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) {
    std::printf("no device: %s\n", vgx_last_error(nullptr));
    return 3;
  }
  int rc = 0;
  vgx_submap gt = nullptr;
  if (vgx_submap_create(ctx, 100, vs, vps, gt_nb, gt_bi.data(), gt_d.data(), gt_w.data(), nullptr, nullptr, &gt) != VGX_OK) {
    std::printf("vgx_submap_create: %s\n", vgx_last_error(ctx));
    rc = 4;
  } else {
    voxgraph_amd::GpuSubmapRegistry::instance().setContext(ctx);
    const voxgraph_amd::GpuMapEvaluation evaluation(ctx, gt, vs, vps);
    const auto r = evaluation.evaluate(collection);
    const auto& d = r.details;
    std::printf("POSE %.17g %.17g %.17g %.17g ITERATIONS %d\n", r.aligned_pose[0], r.aligned_pose[1], r.aligned_pose[2],
                r.aligned_pose[3], r.solver_iterations);
    std::printf("T_GT_READING");
    for (double v : r.T_ground_truth__reading) std::printf(" %.17g", v);
    std::printf("\nDETAILS %a %a %a %a %a %lld %lld %lld %lld\n", d.rmse, d.max_error, d.min_error, d.total_squared_error,
                d.min_abs_error, static_cast<long long>(d.num_evaluated_voxels), static_cast<long long>(d.num_ignored_voxels),
                static_cast<long long>(d.num_overlapping_voxels), static_cast<long long>(d.num_non_overlapping_voxels));
    voxgraph_amd::GpuSubmapRegistry::instance().clear();
    vgx_submap_destroy(gt);
  }
  vgx_ctx_destroy(ctx);
  if (rc == 0) std::printf("MAP_EVAL_SMOKE_OK\n");
  return rc;
}
