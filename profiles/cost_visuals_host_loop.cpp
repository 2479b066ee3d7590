// The route to the cost-function visuals before vgx_reg_evaluate_visuals existed: a plain single-thread loop over the
// f64 rows vgx_reg_evaluate returned and the reference submap's points, building the same three arrays on the host
// (from the SCALED rows: this cannot reproduce the reference's bits; it is the cost that is compared).  Built by
// profiles/cost_visuals_bench.py.
#include <cstdint>
#include <cstring>

namespace {
inline void rotate_translate(float qw, float qz, const float t[3], const float v[3], float out[3]) {
  float uv0 = -(qz * v[1]), uv1 = qz * v[0];
  uv0 += uv0;
  uv1 += uv1;
  const float c0 = -(qz * uv1), c1 = qz * uv0;
  out[0] = (v[0] + qw * uv0 + c0) + t[0];
  out[1] = (v[1] + qw * uv1 + c1) + t[1];
  out[2] = v[2] + t[2];
}
}  // namespace

// rel / mission: {qw, qz, tx, ty, tz} of T_reading__reference and T_mission__reading
extern "C" void cost_visuals_host_loop(int64_t n, const float* xyz, const double* r, const double* jac_read, double factor,
                                       const float* rel, const float* mission, uint8_t* cloud, double* arrows,
                                       double* origins) {
  const double scale = factor * 0.05;
  for (int64_t i = 0; i < n; ++i) {
    float p_read[3], p_m[3];
    rotate_translate(rel[0], rel[1], rel + 2, xyz + 3 * i, p_read);
    rotate_translate(mission[0], mission[1], mission + 2, p_read, p_m);
    float rec[8] = {p_m[0], p_m[1], p_m[2], 1.0f, static_cast<float>(r[i]), 0.0f, 0.0f, 0.0f};
    std::memcpy(cloud + 32 * i, rec, 32);
    for (int a = 0; a < 3; ++a) {
      const double o = static_cast<double>(p_m[a]);
      origins[3 * i + a] = o;
      arrows[6 * i + a] = o;
      arrows[6 * i + 3 + a] = (jac_read[4 * i + a] / factor) * scale + o;
    }
  }
}
