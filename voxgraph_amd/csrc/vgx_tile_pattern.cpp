// vgx_pose_graph_tile_pattern (include/voxgraph_amd.h): the tile structure of the sparse solver for a list of node
// pairs, on the host alone -- no context, no HIP call.
#include <new>

#include "voxgraph_amd.h"
#include "vgx_tile_pattern.h"

extern "C" VGX_API int vgx_pose_graph_tile_pattern(int32_t n_free_nodes, int32_t n_pairs, const int32_t* pairs, int32_t ordering,
                                                   const int32_t* permutation, int32_t* permutation_out, int32_t capacity,
                                                   int32_t* tiles, int32_t* n_tiles) {
  if (n_free_nodes < 1 || n_pairs < 0 || capacity < 0 || (capacity > 0 && !tiles)) return VGX_ERR_INVALID;
  vgx::TileStructure S;
  try {
    if (!vgx::build_tile_structure(n_free_nodes, n_pairs, pairs, ordering, permutation, &S)) return VGX_ERR_INVALID;
  } catch (const std::bad_alloc&) {
    return VGX_ERR_NOMEM;
  }
  if (permutation_out)
    for (int32_t i = 0; i < n_free_nodes; ++i) permutation_out[i] = S.order[(size_t)i];
  if (n_tiles) *n_tiles = (int32_t)S.l_row.size();
  for (size_t t = 0; t < S.l_row.size() && t < (size_t)capacity; ++t) {
    tiles[2 * t] = S.l_row[t];
    tiles[2 * t + 1] = S.l_col[t];
  }
  return VGX_OK;
}
