// GpuEsdfMap / GpuTsdfMap (voxgraph_amd/cpp/gpu_esdf_map.h) from plain C++: the batch forms over one submap, their
// outputs written for tests/test_map_query_cpp.py to compare with the Python path, and the caller's values checked to
// survive every invalid query.
//   map_query_smoke IN OUT
// IN: int32 vps, n_blocks; f32 voxel_size; int32 block_index [nb][3]; f32 tsdf_d, tsdf_w, esdf_d [nb][vps^3]; u8 esdf_o
//     [nb][vps^3]; int64 n; f64 positions [n][3]; f32 T_Q_S [7]
// OUT, in order: ESDF distance + gradient (f64 [n], [n][3], int32 observed [n]); the same posed by T_Q_S; TSDF nearest
//     distance (f64 [n], int32 [n]); TSDF weight (f64 [n], int32 [n]); isObserved on the ESDF (int32 [n])
#include <cstdio>
#include <cstring>
#include <vector>

#include "gpu_esdf_map.h"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) {
  return fread(p, sizeof(T), n, f) == n;
}
template <class T>
void wr(FILE* f, const std::vector<T>& v) {
  fwrite(v.data(), sizeof(T), v.size(), f);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t vps = 0, nb = 0;
  float vs = 0;
  if (!rd(in, &vps, 1) || !rd(in, &nb, 1) || !rd(in, &vs, 1)) return 3;
  const size_t nv = (size_t)nb * vps * vps * vps;
  std::vector<int32_t> bi(3 * (size_t)nb);
  std::vector<float> td(nv), tw(nv), ed(nv);
  std::vector<uint8_t> eo(nv);
  int64_t n = 0;
  if (!rd(in, bi.data(), bi.size()) || !rd(in, td.data(), nv) || !rd(in, tw.data(), nv) || !rd(in, ed.data(), nv) ||
      !rd(in, eo.data(), nv) || !rd(in, &n, 1))
    return 3;
  std::vector<double> pos(3 * (size_t)n);
  float T[7];
  if (!rd(in, pos.data(), pos.size()) || !rd(in, T, 7)) return 3;
  fclose(in);

  vgx_ctx ctx = nullptr;
  if (vgx_ctx_create(0, &ctx) != VGX_OK) return 4;
  vgx_submap sm = nullptr;
  if (vgx_submap_create(ctx, 0, vs, vps, nb, bi.data(), td.data(), tw.data(), ed.data(), eo.data(), &sm) != VGX_OK) return 5;
  voxgraph_amd::GpuEsdfMap esdf(ctx, sm);
  voxgraph_amd::GpuTsdfMap tsdf(ctx, sm);
  const double kSentinel = 12345.5, kGradSentinel = -777.25;
  int bad = 0;
  auto sentinels = [&](const std::vector<double>& v, const std::vector<int>& obs, double s, int per) {
    for (int64_t i = 0; i < n; ++i)
      if (!obs[(size_t)i])
        for (int a = 0; a < per; ++a) bad += v[(size_t)(per * i + a)] != s;
  };
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 2;
  for (int posed = 0; posed < 2; ++posed) {
    esdf.setPose(posed ? T : nullptr);
    std::vector<double> d((size_t)n, kSentinel), g(3 * (size_t)n, kGradSentinel);
    std::vector<int> obs((size_t)n, 7);
    esdf.batchGetDistanceAndGradientAtPosition(n, pos.data(), d.data(), g.data(), obs.data());
    sentinels(d, obs, kSentinel, 1);
    sentinels(g, obs, kGradSentinel, 3);
    wr(out, d);
    wr(out, g);
    wr(out, std::vector<int32_t>(obs.begin(), obs.end()));
  }
  esdf.setPose(nullptr);
  {
    std::vector<double> d((size_t)n, kSentinel);
    std::vector<int> obs((size_t)n, 7);
    for (int64_t i = 0; i < n; ++i) obs[(size_t)i] = tsdf.getDistanceAtPosition(&pos[3 * (size_t)i], false, &d[(size_t)i]);
    sentinels(d, obs, kSentinel, 1);
    wr(out, d);
    wr(out, std::vector<int32_t>(obs.begin(), obs.end()));
    std::vector<double> w((size_t)n, kSentinel);
    tsdf.batchGetWeightAtPosition(n, pos.data(), w.data(), obs.data());
    sentinels(w, obs, kSentinel, 1);
    wr(out, w);
    wr(out, std::vector<int32_t>(obs.begin(), obs.end()));
    esdf.batchIsObserved(n, pos.data(), obs.data());
    wr(out, std::vector<int32_t>(obs.begin(), obs.end()));
  }
  fclose(out);
  // the short forms agree with the batch forms on the first point
  double d1 = kSentinel, g1[3] = {0, 0, 0};
  std::vector<double> db(1, kSentinel), gb(3, 0.0);
  std::vector<int> ob(1, 0);
  const bool ok1 = esdf.getDistanceAndGradientAtPosition(pos.data(), &d1, g1);
  esdf.batchGetDistanceAndGradientAtPosition(1, pos.data(), db.data(), gb.data(), ob.data());
  bad += ok1 != (ob[0] != 0) || d1 != db[0] || std::memcmp(g1, gb.data(), sizeof(g1)) != 0;
  vgx_submap_destroy(sm);
  vgx_ctx_destroy(ctx);
  if (bad) {
    printf("MAP_QUERY_SMOKE_FAILED %d\n", bad);
    return 1;
  }
  printf("MAP_QUERY_SMOKE_OK\n");
  return 0;
}
