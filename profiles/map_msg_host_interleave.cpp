// The host pass a caller needs without vgx_tsdf_layer_serialize / vgx_submap_serialize_layer: the arrays that
// vgx_tsdf_layer_download / vgx_submap_download_layers return, interleaved into voxblox's block words as one plain
// single-thread loop.  The baseline of profiles/map_msg_bench.py; built by it with g++ -O2.  Same words as
// include/voxgraph_amd.h ("Map messages").
#include <cstdint>
#include <cstring>

extern "C" void interleave_tsdf(const float* distance, const float* weight, const uint8_t* rgba /* or NULL */, int64_t n_voxels,
                                uint32_t* words) {
  for (int64_t i = 0; i < n_voxels; ++i) {
    std::memcpy(&words[3 * i], &distance[i], 4);
    std::memcpy(&words[3 * i + 1], &weight[i], 4);
    const uint8_t* c = rgba ? rgba + 4 * i : nullptr;
    words[3 * i + 2] = c ? ((uint32_t)c[3] | (uint32_t)c[2] << 8 | (uint32_t)c[1] << 16 | (uint32_t)c[0] << 24) : 0u;
  }
}

extern "C" void interleave_esdf(const float* distance, const uint8_t* observed, int64_t n_voxels, uint32_t* words) {
  for (int64_t i = 0; i < n_voxels; ++i) {
    std::memcpy(&words[2 * i], &distance[i], 4);
    words[2 * i + 1] = observed[i] ? 1u : 0u;
  }
}
