// cblox::SubmapCollection::getProjectedMap() on the GPU.
//
// voxgraph asks for the projected map in two places (projected_map_server.cpp:31 after every optimisation,
// map_evaluation.cpp:72-73 for evaluation): every submap's TSDF layer resampled into the mission frame at its pose and
// merged into one layer (voxblox mergeLayerAintoLayerB, submaps in ascending ID order).  This header is the swap:
//
//   voxgraph_amd::GpuTsdfLayer gpu_layer(ctx, voxel_size, voxels_per_side);
//   voxgraph_amd::GetProjectedMapOnGpu(submap_collection, &gpu_layer);
//   voxblox::Layer<voxblox::TsdfVoxel> projected_map(voxel_size, voxels_per_side);
//   voxgraph_amd::DownloadTsdfLayer(gpu_layer, &projected_map);                  (gpu_tsdf_layer_bridge.h)
//
// The submaps' device copies come from GpuSubmapRegistry (uploaded on first use, with their raw TSDF layers kept: the
// projection reads them -- a submap whose raw layers were released is refused).  Semantics and deviations (rgba is not
// blended) are stated at vgx_tsdf_layer_merge_submaps in include/voxgraph_amd.h.
#ifndef VOXGRAPH_AMD_CPP_GPU_PROJECTED_MAP_H_
#define VOXGRAPH_AMD_CPP_GPU_PROJECTED_MAP_H_

#include <stdexcept>
#include <string>
#include <vector>

#include "gpu_fast_tsdf_integrator.h"
#include "gpu_submap_registry.h"

namespace voxgraph_amd {

// collection: cblox::SubmapCollection<SubmapT> (getIDs() in ascending order, getSubmapConstPtr(id), and the submaps'
// getPose()).  gpu_layer is emptied and receives the projected map; returned for chaining.
template <typename CollectionT>
GpuTsdfLayer& GetProjectedMapOnGpu(const CollectionT& collection, GpuTsdfLayer* gpu_layer) {
  if (!gpu_layer) throw std::invalid_argument("GetProjectedMapOnGpu: gpu_layer == nullptr");
  GpuSubmapRegistry& registry = GpuSubmapRegistry::instance();
  std::vector<vgx_submap> handles;
  std::vector<float> T_L_S;
  for (const auto id : collection.getIDs()) {  // cblox keeps its submaps in a std::map: ascending IDs
    const auto submap_ptr = collection.getSubmapConstPtr(id);
    handles.push_back(registry.handleOf(submap_ptr));
    const auto& pose = submap_ptr->getPose();
    const auto& q = pose.getRotation();
    const auto& t = pose.getPosition();
    const float T[7] = {static_cast<float>(q.w()), static_cast<float>(q.x()), static_cast<float>(q.y()),
                        static_cast<float>(q.z()), static_cast<float>(t[0]),  static_cast<float>(t[1]),
                        static_cast<float>(t[2])};
    T_L_S.insert(T_L_S.end(), T, T + 7);
  }
  if (vgx_tsdf_layer_upload(gpu_layer->handle(), 0, nullptr, nullptr, nullptr, nullptr) != VGX_OK)
    throw std::runtime_error(std::string("vgx_tsdf_layer_upload: ") + gpu_layer->last_error());
  if (vgx_tsdf_layer_merge_submaps(gpu_layer->handle(), static_cast<int32_t>(handles.size()), handles.data(),
                                   T_L_S.data(), nullptr) != VGX_OK)
    throw std::runtime_error(std::string("vgx_tsdf_layer_merge_submaps: ") + gpu_layer->last_error());
  return *gpu_layer;
}

}  // namespace voxgraph_amd

#endif  // VOXGRAPH_AMD_CPP_GPU_PROJECTED_MAP_H_
