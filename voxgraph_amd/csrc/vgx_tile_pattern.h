// Pose graph: the tile structure of the sparse Cholesky (include/voxgraph_amd.h, "Pose graph: the tile-sparse solver").
// Pure host C++, no HIP: the block graph over the free nodes, its ordering, the 64 x 64 tiles of H that some 4x4 block
// touches, the symbolic fill of L at tile granularity and the per-panel lists the kernels walk.  Header-only, so that a
// stand-alone program can run it under a sanitizer (tests/cpp/tile_pattern_check.cpp).
#ifndef VGX_TILE_PATTERN_H_
#define VGX_TILE_PATTERN_H_
#include <algorithm>
#include <cstdint>
#include <set>
#include <utility>
#include <vector>

namespace vgx {

constexpr int kTile = 64;            // tile size = panel width of the factorisation
constexpr int kNodesPerTile = 16;    // 4 unknowns per node
constexpr int kOrderNatural = 0, kOrderRcm = 1, kOrderGiven = 2;

struct TileTriple {
  int32_t target, source_i, source_j;  // L tile indices: (I, J) -= (I, K) (J, K)^T
  int32_t rows;                        // rows of tile row I | rows of tile row J << 8 | (I == J) << 16
};

struct TileStructure {
  int32_t n_free = 0, n_tile_rows = 0;
  std::vector<int32_t> order;      // position -> free node
  std::vector<int32_t> position;   // free node -> position
  // L: tiles sorted by (column, row); column K is [col_first[K], col_first[K + 1]), its first tile the diagonal one
  std::vector<int32_t> l_row, l_col, col_first;
  // ... and per tile row K its tiles left of the diagonal, ascending column: indices into the list above
  std::vector<int32_t> row_first, row_tile, row_col;
  // the trailing updates of panel K: [triple_first[K], triple_first[K + 1])
  std::vector<int64_t> triple_first;
  std::vector<TileTriple> triples;
  // H: both triangles, sorted by (row, column); row I is [h_row_first[I], h_row_first[I + 1])
  std::vector<int32_t> h_row_first, h_col, h_diag;
  std::vector<int32_t> l_from_h;   // per L tile: the H tile it starts as a copy of, or -1 (pure fill: starts at +0.0)

  int32_t rows_of(int32_t tile_row) const { return std::min(kTile, 4 * n_free - kTile * tile_row); }
  // the L tile (I, J), I >= J; -1 when it is not stored
  int32_t l_tile(int32_t I, int32_t J) const {
    const auto b = l_row.begin() + col_first[(size_t)J], e = l_row.begin() + col_first[(size_t)J + 1];
    const auto it = std::lower_bound(b, e, I);
    return (it != e && *it == I) ? (int32_t)(it - l_row.begin()) : -1;
  }
};

// true when `perm` [n] holds every value of [0, n) once
inline bool is_permutation(const int32_t* perm, int32_t n) {
  if (n < 0 || (n > 0 && !perm)) return false;
  std::vector<char> seen((size_t)n, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (perm[i] < 0 || perm[i] >= n || seen[(size_t)perm[i]]) return false;
    seen[(size_t)perm[i]] = 1;
  }
  return true;
}

// Reverse Cuthill-McKee on the block graph, deterministic: components in ascending order of their lowest node, each
// started at its minimum-degree node (ties: the lowest index), breadth-first, a node's unvisited neighbours appended
// by ascending (degree, index); the whole sequence reversed.
inline std::vector<int32_t> rcm_order(int32_t n, const std::vector<std::vector<int32_t>>& adj) {
  std::vector<int32_t> seq;
  seq.reserve((size_t)n);
  std::vector<char> in_component((size_t)n, 0), visited((size_t)n, 0);
  std::vector<int32_t> component, next;
  for (int32_t v = 0; v < n; ++v) {
    if (in_component[(size_t)v]) continue;
    component.assign(1, v);
    in_component[(size_t)v] = 1;
    for (size_t h = 0; h < component.size(); ++h)
      for (int32_t u : adj[(size_t)component[h]])
        if (!in_component[(size_t)u]) {
          in_component[(size_t)u] = 1;
          component.push_back(u);
        }
    int32_t start = component[0];
    for (int32_t u : component)
      if (adj[(size_t)u].size() < adj[(size_t)start].size() || (adj[(size_t)u].size() == adj[(size_t)start].size() && u < start)) start = u;
    size_t head = seq.size();
    seq.push_back(start);
    visited[(size_t)start] = 1;
    for (; head < seq.size(); ++head) {
      next.clear();
      for (int32_t u : adj[(size_t)seq[head]])
        if (!visited[(size_t)u]) {
          visited[(size_t)u] = 1;
          next.push_back(u);
        }
      std::sort(next.begin(), next.end(), [&](int32_t a, int32_t b) {
        return adj[(size_t)a].size() != adj[(size_t)b].size() ? adj[(size_t)a].size() < adj[(size_t)b].size() : a < b;
      });
      seq.insert(seq.end(), next.begin(), next.end());
    }
  }
  std::reverse(seq.begin(), seq.end());
  return seq;
}

// pairs [n_pairs][2]: free nodes (in the graph's order) that a constraint joins; a pair of a node with itself is
// allowed and adds nothing.  given: the caller's order for kOrderGiven (position -> free node).  false: a pair out of
// range, an unknown ordering, a `given` that is no permutation, n_free < 0.
inline bool build_tile_structure(int32_t n_free, int64_t n_pairs, const int32_t* pairs, int32_t ordering, const int32_t* given,
                                 TileStructure* out) {
  TileStructure& S = *out;
  S = TileStructure();
  if (n_free < 0 || n_pairs < 0 || (n_pairs > 0 && !pairs)) return false;
  if (ordering != kOrderNatural && ordering != kOrderRcm && ordering != kOrderGiven) return false;
  for (int64_t p = 0; p < 2 * n_pairs; ++p)
    if (pairs[p] < 0 || pairs[p] >= n_free) return false;
  if (ordering == kOrderGiven && !is_permutation(given, n_free)) return false;
  S.n_free = n_free;
  const int32_t nT = S.n_tile_rows = (n_free + kNodesPerTile - 1) / kNodesPerTile;
  if (ordering == kOrderRcm) {
    std::vector<std::vector<int32_t>> adj((size_t)n_free);
    for (int64_t p = 0; p < n_pairs; ++p) {
      const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
      if (a == b) continue;
      adj[(size_t)a].push_back(b);
      adj[(size_t)b].push_back(a);
    }
    for (auto& list : adj) {
      std::sort(list.begin(), list.end());
      list.erase(std::unique(list.begin(), list.end()), list.end());
    }
    S.order = rcm_order(n_free, adj);
  } else {
    S.order.resize((size_t)n_free);
    for (int32_t i = 0; i < n_free; ++i) S.order[(size_t)i] = ordering == kOrderGiven ? given[i] : i;
  }
  S.position.assign((size_t)n_free, 0);
  for (int32_t p = 0; p < n_free; ++p) S.position[(size_t)S.order[(size_t)p]] = p;

  // the tiles of H (lower triangle, by column), then the fill: K ascending, every I >= J > K of column K joins column J
  std::vector<std::set<int32_t>> column((size_t)nT);
  for (int32_t K = 0; K < nT; ++K) column[(size_t)K].insert(K);
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int32_t ta = S.position[(size_t)pairs[2 * p]] / kNodesPerTile, tb = S.position[(size_t)pairs[2 * p + 1]] / kNodesPerTile;
    column[(size_t)std::min(ta, tb)].insert(std::max(ta, tb));
  }
  std::vector<std::vector<int32_t>> h_lower((size_t)nT);
  for (int32_t K = 0; K < nT; ++K) h_lower[(size_t)K].assign(column[(size_t)K].begin(), column[(size_t)K].end());
  std::vector<int32_t> below;
  for (int32_t K = 0; K < nT; ++K) {
    below.assign(std::next(column[(size_t)K].begin()), column[(size_t)K].end());
    for (size_t j = 0; j < below.size(); ++j)
      for (size_t i = j + 1; i < below.size(); ++i) column[(size_t)below[j]].insert(below[i]);
  }
  S.col_first.assign((size_t)nT + 1, 0);
  for (int32_t K = 0; K < nT; ++K) {
    for (int32_t I : column[(size_t)K]) {
      S.l_row.push_back(I);
      S.l_col.push_back(K);
    }
    S.col_first[(size_t)K + 1] = (int32_t)S.l_row.size();
  }
  // row lists
  std::vector<std::vector<std::pair<int32_t, int32_t>>> rows((size_t)nT);
  for (size_t t = 0; t < S.l_row.size(); ++t)
    if (S.l_row[t] != S.l_col[t]) rows[(size_t)S.l_row[t]].push_back({S.l_col[t], (int32_t)t});  // (by column, so ascending)
  S.row_first.assign((size_t)nT + 1, 0);
  for (int32_t K = 0; K < nT; ++K) {
    for (const auto& e : rows[(size_t)K]) {
      S.row_col.push_back(e.first);
      S.row_tile.push_back(e.second);
    }
    S.row_first[(size_t)K + 1] = (int32_t)S.row_tile.size();
  }
  // update triples
  S.triple_first.assign((size_t)nT + 1, 0);
  for (int32_t K = 0; K < nT; ++K) {
    const int32_t first = S.col_first[(size_t)K], last = S.col_first[(size_t)K + 1];
    for (int32_t tj = first + 1; tj < last; ++tj)
      for (int32_t ti = tj; ti < last; ++ti) {
        const int32_t I = S.l_row[(size_t)ti], J = S.l_row[(size_t)tj];
        S.triples.push_back({S.l_tile(I, J), ti, tj, S.rows_of(I) | S.rows_of(J) << 8 | (I == J) << 16});
      }
    S.triple_first[(size_t)K + 1] = (int64_t)S.triples.size();
  }
  // H: both triangles by row
  std::vector<std::vector<int32_t>> h_rows((size_t)nT);
  for (int32_t K = 0; K < nT; ++K)
    for (int32_t I : h_lower[(size_t)K]) {
      h_rows[(size_t)I].push_back(K);
      if (I != K) h_rows[(size_t)K].push_back(I);
    }
  S.h_row_first.assign((size_t)nT + 1, 0);
  S.h_diag.assign((size_t)nT, 0);
  for (int32_t I = 0; I < nT; ++I) {
    std::sort(h_rows[(size_t)I].begin(), h_rows[(size_t)I].end());
    for (int32_t J : h_rows[(size_t)I]) {
      if (J == I) S.h_diag[(size_t)I] = (int32_t)S.h_col.size();
      S.h_col.push_back(J);
    }
    S.h_row_first[(size_t)I + 1] = (int32_t)S.h_col.size();
  }
  S.l_from_h.assign(S.l_row.size(), -1);
  for (size_t t = 0; t < S.l_row.size(); ++t) {
    const int32_t I = S.l_row[t], J = S.l_col[t];
    const auto b = S.h_col.begin() + S.h_row_first[(size_t)I], e = S.h_col.begin() + S.h_row_first[(size_t)I + 1];
    const auto it = std::lower_bound(b, e, J);
    if (it != e && *it == J) S.l_from_h[t] = (int32_t)(it - S.h_col.begin());
  }
  return true;
}

// the H tile (I, J) of a structure; -1 when it is not stored
inline int32_t h_tile(const TileStructure& S, int32_t I, int32_t J) {
  const auto b = S.h_col.begin() + S.h_row_first[(size_t)I], e = S.h_col.begin() + S.h_row_first[(size_t)I + 1];
  const auto it = std::lower_bound(b, e, J);
  return (it != e && *it == J) ? (int32_t)(it - S.h_col.begin()) : -1;
}

}  // namespace vgx
#endif  // VGX_TILE_PATTERN_H_
