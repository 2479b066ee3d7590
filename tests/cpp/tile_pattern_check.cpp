// The tile structure code (voxgraph_amd/csrc/vgx_tile_pattern.h) in a program of its own, to be built with
// -fsanitize=address,undefined and no HIP (tests/test_pose_graph_sparse_cpu.py): the pattern scenes of the CPU tests under
// the three orderings, the invariants of the lists, malformed input, and a seeded sweep of a few thousand random structures of
// the fuzzer's families (profiles/fuzz_pose_graph_scene.py).  Prints "tile_pattern_check ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "vgx_tile_pattern.h"

using namespace vgx;

#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

static void check_structure(int32_t n, const std::vector<int32_t>& pairs, int32_t ordering, const int32_t* given) {
  TileStructure S;
  CHECK(build_tile_structure(n, (int64_t)pairs.size() / 2, pairs.data(), ordering, given, &S));
  CHECK(is_permutation(S.order.data(), n));
  const int32_t nT = S.n_tile_rows;
  CHECK((int32_t)S.col_first.size() == nT + 1 && S.col_first[(size_t)nT] == (int32_t)S.l_row.size());
  for (int32_t K = 0; K < nT; ++K) {
    CHECK(S.l_row[(size_t)S.col_first[(size_t)K]] == K);                       // the diagonal tile leads its column
    for (int32_t t = S.col_first[(size_t)K] + 1; t < S.col_first[(size_t)K + 1]; ++t) CHECK(S.l_row[(size_t)t] > S.l_row[(size_t)t - 1]);
    CHECK(S.h_col[(size_t)S.h_diag[(size_t)K]] == K);
  }
  for (int64_t p = 0; p < (int64_t)pairs.size() / 2; ++p) {                    // every joined pair has its tiles
    const int32_t a = S.position[(size_t)pairs[2 * p]] / kNodesPerTile, b = S.position[(size_t)pairs[2 * p + 1]] / kNodesPerTile;
    CHECK(S.l_tile(std::max(a, b), std::min(a, b)) >= 0 && h_tile(S, a, b) >= 0 && h_tile(S, b, a) >= 0);
  }
  const int32_t n_tiles = (int32_t)S.l_row.size();
  for (const TileTriple& t : S.triples) {                                      // closed under the fill rule
    // (a fill tile missing from the list would make l_tile answer -1: the kernel's target would lie before the array)
    CHECK(t.target >= 0 && t.target < n_tiles && t.source_i >= 0 && t.source_i < n_tiles && t.source_j >= 0 && t.source_j < n_tiles);
    CHECK(S.l_tile(S.l_row[(size_t)t.source_i], S.l_row[(size_t)t.source_j]) == t.target);
    CHECK(t.rows == (S.rows_of(S.l_row[(size_t)t.source_i]) | S.rows_of(S.l_row[(size_t)t.source_j]) << 8 |
                     (S.l_row[(size_t)t.source_i] == S.l_row[(size_t)t.source_j]) << 16));
    CHECK((t.rows & 255) >= 4 && ((t.rows >> 8) & 255) >= 4 && (t.rows & 255) <= kTile && (t.rows & 3) == 0);
    CHECK(S.l_row[(size_t)t.target] == S.l_row[(size_t)t.source_i] && S.l_col[(size_t)t.target] == S.l_row[(size_t)t.source_j]);
    CHECK(S.l_col[(size_t)t.source_i] == S.l_col[(size_t)t.source_j] && S.l_col[(size_t)t.source_i] < S.l_col[(size_t)t.target]);
    CHECK((t.rows & 255) == S.rows_of(S.l_row[(size_t)t.target]) && ((t.rows >> 8) & 255) == S.rows_of(S.l_col[(size_t)t.target]));
  }
  CHECK(S.triple_first[(size_t)nT] == (int64_t)S.triples.size() && S.row_first[(size_t)nT] == (int32_t)S.row_tile.size());
  for (size_t q = 0; q < S.row_tile.size(); ++q) CHECK(S.l_col[(size_t)S.row_tile[q]] == S.row_col[q]);
  size_t from_h = 0;
  for (int32_t v : S.l_from_h) from_h += v >= 0;
  CHECK(2 * from_h - (size_t)nT == S.h_col.size());
}

// ---- the seeded sweep: a small generator of its own, so that every platform draws the same structures ----
struct Lcg {
  uint64_t state;
  uint32_t next() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
  }
  int32_t below(int32_t n) { return (int32_t)(next() % (uint32_t)n); }        // n >= 1
  bool chance(int percent) { return below(100) < percent; }
};

// family 0 .. 8: empty, chain, chain with second neighbours, random pairs, hub, arrow, band with closures, components with
// isolated nodes, a chain relabelled by a random permutation -- in either direction, then repeated pairs and a node with itself
static std::vector<int32_t> random_pairs(Lcg& r, int family, int32_t n) {
  std::vector<int32_t> p;
  auto join = [&](int32_t a, int32_t b) {
    if (r.chance(50)) std::swap(a, b);
    p.insert(p.end(), {a, b});
  };
  if (n >= 2) {
    if (family == 1 || family == 2) {
      for (int32_t i = 0; i + 1 < n; ++i) join(i + 1, i);
      if (family == 2)
        for (int32_t i = 0; i + 2 < n; ++i) join(i + 2, i);
    } else if (family == 3) {
      const int32_t count = n * (1 + r.below(8)) / 2;
      for (int32_t k = 0; k < count; ++k) join(r.below(n), r.below(n));        // (a node with itself among them)
    } else if (family == 4) {
      const int32_t at[4] = {0, n / 2, n - 1, r.below(n)};
      const int32_t hub = at[r.below(4)];
      const int percent = 30 + r.below(60);
      for (int32_t i = 0; i < n; ++i)
        if (i != hub && r.chance(percent)) join(hub, i);
      if (r.chance(50))
        for (int32_t i = 0; i + 1 < n; ++i) join(i + 1, i);
    } else if (family == 5) {
      for (int32_t i = 1; i < n; ++i) join(i, 0);
    } else if (family == 6) {
      const int32_t width = 1 + r.below(3);
      for (int32_t w = 1; w <= width; ++w)
        for (int32_t i = 0; i + w < n; ++i) join(i + w, i);
      for (int32_t k = r.below(4); k >= 0; --k) join(r.below(n), r.below(n));
    } else if (family == 7) {
      int32_t last = -1;
      for (int32_t i = 0; i < n; ++i) {
        if (r.chance(4)) last = -1;                                             // a new component starts
        if (r.chance(15)) continue;                                             // an isolated node
        if (last >= 0) join(last, i);
        last = i;
      }
    } else if (family == 8) {
      std::vector<int32_t> label((size_t)n);
      std::iota(label.begin(), label.end(), 0);
      for (int32_t i = n - 1; i > 0; --i) std::swap(label[(size_t)i], label[(size_t)r.below(i + 1)]);
      for (int32_t i = 0; i + 1 < n; ++i) join(label[(size_t)i + 1], label[(size_t)i]);
    }
  }
  if (!p.empty() && r.chance(50))
    for (int k = 0; k < 3; ++k) {
      const size_t q = 2 * (size_t)r.below((int32_t)(p.size() / 2));
      p.insert(p.end(), {p[q], p[q + 1]});                                      // a repeated pair
    }
  if (r.chance(30)) {
    const int32_t v = r.below(n);
    p.insert(p.end(), {v, v});                                                  // a node with itself
  }
  return p;
}

static void sweep(int n_structures) {
  Lcg r{20240607};
  const int32_t sizes[] = {1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 130};
  for (int k = 0; k < n_structures; ++k) {
    const int family = k % 9;
    const int32_t n = (k % 12 == 11) ? 280 + r.below(51) : sizes[r.below((int32_t)(sizeof(sizes) / sizeof(sizes[0])))];
    const std::vector<int32_t> pairs = random_pairs(r, family, n);
    std::vector<int32_t> given((size_t)n);
    std::iota(given.begin(), given.end(), 0);
    for (int32_t i = n - 1; i > 0; --i) std::swap(given[(size_t)i], given[(size_t)r.below(i + 1)]);
    check_structure(n, pairs, kOrderNatural, nullptr);
    check_structure(n, pairs, kOrderRcm, nullptr);
    check_structure(n, pairs, kOrderGiven, given.data());
  }
}

int main() {
  std::vector<std::pair<int32_t, std::vector<int32_t>>> scenes;
  {
    std::vector<int32_t> chain, chain2, hub, two;
    for (int i = 0; i + 1 < 100; ++i) chain.insert(chain.end(), {i + 1, i});
    for (int i = 0; i + 1 < 150; ++i) chain2.insert(chain2.end(), {i + 1, i});
    for (int i = 0; i + 2 < 150; ++i) chain2.insert(chain2.end(), {i + 2, i});
    chain2.insert(chain2.end(), {140, 5, 90, 40});
    for (int i = 0; i + 1 < 77; ++i) hub.insert(hub.end(), {i, i + 1});
    for (int i = 8; i < 77; i += 2) hub.insert(hub.end(), {i % 4 ? 4 : i, i % 4 ? i : 4});
    hub.insert(hub.end(), {10, 9, 4, 4});                                      // an edge twice over, a node with itself
    for (int i = 0; i + 1 < 40; ++i) two.insert(two.end(), {i + 1, i});
    for (int i = 41; i + 1 < 89; ++i) two.insert(two.end(), {i + 1, i});
    two.insert(two.end(), {88, 45, 30, 2});
    scenes = {{100, chain}, {150, chain2}, {77, hub}, {90, two}, {1, {}}, {16, {}}, {17, {16, 0}}, {4200, {}}};
    for (int i = 0; i + 2 < 4200; ++i) scenes.back().second.insert(scenes.back().second.end(), {i, i + 1, i + 2, i});
    scenes.back().second.insert(scenes.back().second.end(), {4100, 30, 2000, 900});
  }
  std::mt19937 rng(7);
  for (const auto& scene : scenes) {
    const int32_t n = scene.first;
    std::vector<int32_t> given((size_t)n);
    std::iota(given.begin(), given.end(), 0);
    std::shuffle(given.begin(), given.end(), rng);
    check_structure(n, scene.second, kOrderNatural, nullptr);
    check_structure(n, scene.second, kOrderRcm, nullptr);
    check_structure(n, scene.second, kOrderGiven, given.data());
  }
  sweep(3000);
  // malformed input is refused, not read past
  TileStructure S;
  const int32_t repeat[4] = {0, 1, 1, 3}, beyond[4] = {0, 1, 2, 4}, good[4] = {3, 1, 0, 2};
  const int32_t pair_ok[2] = {1, 2}, pair_high[2] = {3, 4}, pair_negative[2] = {-1, 2};
  CHECK(build_tile_structure(4, 1, pair_ok, kOrderGiven, good, &S));
  CHECK(!build_tile_structure(4, 1, pair_ok, kOrderGiven, repeat, &S));
  CHECK(!build_tile_structure(4, 1, pair_ok, kOrderGiven, beyond, &S));
  CHECK(!build_tile_structure(4, 1, pair_ok, kOrderGiven, nullptr, &S));
  CHECK(!build_tile_structure(4, 1, pair_high, kOrderNatural, nullptr, &S));
  CHECK(!build_tile_structure(4, 1, pair_negative, kOrderRcm, nullptr, &S));
  CHECK(!build_tile_structure(4, 1, nullptr, kOrderNatural, nullptr, &S));
  CHECK(!build_tile_structure(4, -1, pair_ok, kOrderNatural, nullptr, &S));
  CHECK(!build_tile_structure(4, 1, pair_ok, 3, nullptr, &S));
  CHECK(!build_tile_structure(-1, 0, nullptr, kOrderNatural, nullptr, &S));
  CHECK(build_tile_structure(0, 0, nullptr, kOrderRcm, nullptr, &S) && S.l_row.empty() && S.order.empty());   // zero free nodes: empty lists
  CHECK(!build_tile_structure(0, 1, pair_ok, kOrderNatural, nullptr, &S));
  std::printf("tile_pattern_check ok\n");
  return 0;
}
