// The layer a voxel-reading product walks, whatever holds it: the source abstraction of the layer clouds (vgx_cloud.hip)
// and the planar map (vgx_planar.hip).  Three layouts (SRC): a finished submap's ESDF (f32 distance + u8 observed) and
// TSDF (f32 distance + f32 weight) layers, and a vgx_tsdf_layer's packed {distance, weight} words with their colours.
#ifndef VGX_CLOUD_SRC_H_
#define VGX_CLOUD_SRC_H_

#include "vgx_internal.h"

namespace vgx {

enum { kCloudSrcEsdf = 0, kCloudSrcTsdf = 1, kCloudSrcPacked = 2 };

struct CloudSrc {
  const int32_t* block_index;  // [slots][3]
  // the layer's block count where only the device knows it when the passes are queued (an active layer's allocation
  // counter, an evaluation's error-block count); null: every slot of the grid is a block
  const void* live_blocks;
  int32_t live_blocks_is_64;
  const float* dist;                // ESDF / TSDF
  const void* seen;                 // ESDF: u8 observed; TSDF: f32 weight
  const unsigned long long* words;  // packed: {distance (lo), weight (hi)}
  const uint32_t* rgba;             // packed
  float voxel_size;
};

__device__ __forceinline__ int cloud_live_blocks(const CloudSrc& s, int slots) {
  if (!s.live_blocks) return slots;
  const long long n = s.live_blocks_is_64 ? *static_cast<const long long*>(s.live_blocks) : (long long)*static_cast<const int32_t*>(s.live_blocks);
  return (int)(n < (long long)slots ? n : (long long)slots);
}

// One voxel, `at` its index in the block pool (slot * vps^3 + linear index): its distance, and whether it is observed --
// ESDF observed != 0; TSDF weight > min_weight, strictly (a NaN weight is not).
template <int SRC>
__device__ __forceinline__ bool cloud_voxel(const CloudSrc& s, size_t at, float min_weight, float* d) {
  if (SRC == kCloudSrcPacked) {
    const unsigned long long w = s.words[at];
    *d = __uint_as_float((uint32_t)w);
    return __uint_as_float((uint32_t)(w >> 32)) > min_weight;
  }
  *d = s.dist[at];
  if (SRC == kCloudSrcTsdf) return static_cast<const float*>(s.seen)[at] > min_weight;
  return static_cast<const uint8_t*>(s.seen)[at] != 0;
}

}  // namespace vgx

#endif
