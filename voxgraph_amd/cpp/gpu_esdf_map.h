// voxblox::EsdfMap / voxblox::TsdfMap queries on the GPU.
//
// A VoxgraphSubmap is a cblox::TsdfEsdfSubmap; planners and other users read voxgraph's map through
// submap.getEsdfMap() / getTsdfMap() and voxblox's query methods [recalled].  GpuEsdfMap and GpuTsdfMap answer the same
// calls, with the same names and results, from a finished submap on the device (vgx_submap_query): a finished submap, or
// the projected map made into one.  The swap where a map is queried:
//
//   voxgraph_amd::GpuEsdfMap esdf(ctx, submap_handle);       // instead of submap.getEsdfMap()
//   double d;  double g[3];
//   if (esdf.getDistanceAndGradientAtPosition(position, &d, g)) ...
//   esdf.batchGetDistanceAtPosition(n, positions, distances, observed);   // n points in one launch
//
// Plain arrays stand in for Eigen's (positions [n][3], gradients [n][3], x fastest; one double[3] per point), as
// voxgraph_submap_bridge.h does.  Positions are cast to f32 once, as EsdfMap does, and results written as doubles.  The
// short forms use voxblox's default interpolate = true [recalled].  On an invalid query the batch forms leave the caller's
// distance and gradient untouched and only observed[i] = 0 says so (voxblox's behaviour; the C ABI writes zeros there).
// Optional T_Q_S {qw,qx,qy,qz, tx,ty,tz}: the positions are in frame Q (the mission frame at the submap's pose) and the
// gradients come back in it.  Semantics: vgx_submap_query in include/voxgraph_amd.h.
#ifndef VOXGRAPH_AMD_CPP_GPU_ESDF_MAP_H_
#define VOXGRAPH_AMD_CPP_GPU_ESDF_MAP_H_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "voxgraph_amd.h"

namespace voxgraph_amd {

// the common part: one layer of one finished submap (the handle stays the caller's)
class GpuLayerMap {
 public:
  GpuLayerMap(vgx_ctx ctx, vgx_submap submap, int32_t layer) : ctx_(ctx), submap_(submap), layer_(layer) {}

  // positions are in frame Q: p_S = T_Q_S^-1 p_Q (NULL: the submap frame, the default)
  void setPose(const float T_Q_S[7]) {
    posed_ = T_Q_S != nullptr;
    if (posed_)
      for (int k = 0; k < 7; ++k) T_Q_S_[k] = T_Q_S[k];
  }

  vgx_submap handle() const { return submap_; }

  bool getDistanceAtPosition(const double position[3], double* distance) const {
    return getDistanceAtPosition(position, true, distance);
  }
  bool getDistanceAtPosition(const double position[3], bool interpolate, double* distance) const {
    int obs = 0;
    batch(1, position, interpolate, false, distance, nullptr, nullptr, &obs);
    return obs != 0;
  }
  bool getDistanceAndGradientAtPosition(const double position[3], double* distance, double gradient[3]) const {
    return getDistanceAndGradientAtPosition(position, true, distance, gradient);
  }
  bool getDistanceAndGradientAtPosition(const double position[3], bool interpolate, double* distance,
                                        double gradient[3]) const {
    int obs = 0;
    batch(1, position, interpolate, true, distance, gradient, nullptr, &obs);
    return obs != 0;
  }
  // the position's own voxel exists and is observed (ESDF observed, TSDF weight > 0)
  bool isObserved(const double position[3]) const {
    int obs = 0;
    double d = 0.0;
    batch(1, position, false, false, &d, nullptr, nullptr, &obs);
    return obs != 0;
  }

  // n positions in one launch; distances [n], observed [n] (1 / 0)
  void batchGetDistanceAtPosition(int64_t n, const double* positions, double* distances, int* observed) const {
    batch(n, positions, true, false, distances, nullptr, nullptr, observed);
  }
  void batchGetDistanceAndGradientAtPosition(int64_t n, const double* positions, double* distances, double* gradients,
                                             int* observed) const {
    batch(n, positions, true, true, distances, gradients, nullptr, observed);
  }
  void batchIsObserved(int64_t n, const double* positions, int* observed) const {
    std::vector<double> scratch((size_t)n);
    batch(n, positions, false, false, scratch.data(), nullptr, nullptr, observed);
  }

 protected:
  // one vgx_submap_query; invalid entries leave distances / gradients / weights untouched
  void batch(int64_t n, const double* positions, bool interpolate, bool want_gradient, double* distances, double* gradients,
             double* weights, int* observed) const {
    if (n <= 0) return;
    std::vector<float> p((size_t)n * 3), d((size_t)n), g(want_gradient ? (size_t)n * 3 : 0), w(weights ? (size_t)n : 0);
    std::vector<uint8_t> v((size_t)n);
    for (size_t i = 0; i < p.size(); ++i) p[i] = (float)positions[i];
    const int32_t flags = (interpolate ? VGX_QUERY_INTERPOLATE : 0) | (want_gradient ? VGX_QUERY_GRADIENT : 0);
    const int rc = vgx_submap_query(submap_, layer_, flags, posed_ ? T_Q_S_ : nullptr, n, p.data(), d.data(),
                                    want_gradient ? g.data() : nullptr, weights ? w.data() : nullptr, v.data());
    if (rc != VGX_OK) throw std::runtime_error(std::string("vgx_submap_query: ") + vgx_last_error(ctx_));
    for (int64_t i = 0; i < n; ++i) {
      observed[i] = v[(size_t)i] ? 1 : 0;
      if (!v[(size_t)i]) continue;
      distances[i] = d[(size_t)i];
      if (want_gradient)
        for (int a = 0; a < 3; ++a) gradients[3 * i + a] = g[3 * (size_t)i + a];
      if (weights) weights[i] = w[(size_t)i];
    }
  }

  vgx_ctx ctx_;
  vgx_submap submap_;
  int32_t layer_;
  bool posed_ = false;
  float T_Q_S_[7] = {1, 0, 0, 0, 0, 0, 0};
};

// voxblox::EsdfMap over a finished submap's ESDF layer (vgx_submap_generate_esdf must have run)
class GpuEsdfMap : public GpuLayerMap {
 public:
  GpuEsdfMap(vgx_ctx ctx, vgx_submap submap) : GpuLayerMap(ctx, submap, VGX_EVAL_LAYER_ESDF) {}
};

// voxblox::TsdfMap over a finished submap's raw TSDF layer
class GpuTsdfMap : public GpuLayerMap {
 public:
  GpuTsdfMap(vgx_ctx ctx, vgx_submap submap) : GpuLayerMap(ctx, submap, VGX_EVAL_LAYER_TSDF) {}

  bool getWeightAtPosition(const double position[3], double* weight) const {
    return getWeightAtPosition(position, true, weight);
  }
  bool getWeightAtPosition(const double position[3], bool interpolate, double* weight) const {
    int obs = 0;
    double d = 0.0;
    batch(1, position, interpolate, false, &d, nullptr, weight, &obs);
    return obs != 0;
  }
  void batchGetWeightAtPosition(int64_t n, const double* positions, double* weights, int* observed) const {
    std::vector<double> scratch((size_t)n);
    batch(n, positions, true, false, scratch.data(), nullptr, weights, observed);
  }
};

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_ESDF_MAP_H_
