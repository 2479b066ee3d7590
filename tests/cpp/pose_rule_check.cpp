// The pose rule (voxgraph_amd/csrc/vgx_pose.h) in a program of its own, built with AddressSanitizer and UBSan by
// tests/test_pose_rule_cpu.py.  It includes nothing else of the library.  Over a seeded table of poses and points it
// prints the f32 bit patterns of quat_rotate, rigid_apply and inverse_pose next to their inputs, and pose_defect's verdict
// for finite, non-finite and nearly-unit poses; the test recomputes every line with tests/projected_map_ref.py.
//
//   R <q: 4 words> <t: 3> <v: 3> <quat_rotate: 3> <rigid_apply: 3> <inverse_pose q: 4> <inverse_pose t: 3>
//   D <T: 7 words> <verdict: 0 none, 1 not finite, 2 not unit>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "vgx_pose.h"

namespace {

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

void put(const float* v, int n) {
  for (int i = 0; i < n; ++i) std::printf(" %08x", bits(v[i]));
}

uint64_t state = 0x9e3779b97f4a7c15ull;
float uniform(float lo, float hi) {  // splitmix64, the top 24 bits
  state += 0x9e3779b97f4a7c15ull;
  uint64_t z = state;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return lo + (hi - lo) * ((float)(z >> 40) / 16777216.0f);
}

void rotate_line(const float q[4], const float t[3], const float v[3]) {
  float rot[3], rig[3], qi[4], ti[3];
  vgx::quat_rotate(q, v, rot);
  vgx::rigid_apply(q, t, v, rig);
  vgx::inverse_pose(q, t, qi, ti);
  std::printf("R");
  put(q, 4);
  put(t, 3);
  put(v, 3);
  put(rot, 3);
  put(rig, 3);
  put(qi, 4);
  put(ti, 3);
  std::printf("\n");
}

void defect_line(const float T[7]) {
  std::printf("D");
  put(T, 7);
  std::printf(" %d\n", (int)vgx::pose_defect(T));
}

}  // namespace

int main() {
  // the identity, the quarter and half turns about the axes, then random rotations of every size
  const float h = std::sqrt(0.5f);
  const float fixed[][4] = {{1, 0, 0, 0}, {h, h, 0, 0}, {h, 0, h, 0}, {h, 0, 0, h}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}, {h, 0, 0, -h}};
  for (const auto& q : fixed) {
    const float zero[3] = {0.0f, 0.0f, 0.0f}, t[3] = {1.5f, -2.25f, 0.125f}, v[3] = {0.3f, -4.0f, 7.7f};
    rotate_line(q, zero, v);
    rotate_line(q, t, v);
  }
  for (int i = 0; i < 400; ++i) {
    float q[4], t[3], v[3];
    float n2 = 0.0f;
    for (int k = 0; k < 4; ++k) {
      q[k] = uniform(-1.0f, 1.0f);
      n2 += q[k] * q[k];
    }
    if (!(n2 > 1e-3f)) continue;
    const float inv = 1.0f / std::sqrt(n2);
    for (int k = 0; k < 4; ++k) q[k] *= inv;
    const float reach = i % 4 == 0 ? 1000.0f : 10.0f;
    for (int a = 0; a < 3; ++a) {
      t[a] = uniform(-reach, reach);
      v[a] = uniform(-2.0f * reach, 2.0f * reach);
    }
    rotate_line(q, t, v);
  }

  // pose_defect: finite unit poses; a non-finite value in every place, also in a pose that is not unit either (not
  // finite wins); |q|^2 around 1 - 1e-4 and 1 + 1e-4 in steps of 1e-7, on both sides of each bound; far from unit
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float unit[7] = {h, 0.0f, -h, 0.0f, 3.0f, -4.0f, 5.0f};
  defect_line(unit);
  for (int k = 0; k < 7; ++k)
    for (float bad : {nan, inf, -inf}) {
      float T[7];
      std::memcpy(T, unit, sizeof(T));
      T[k] = bad;
      defect_line(T);
      T[(k + 1) % 4] = 2.0f;
      defect_line(T);
    }
  for (int side = -1; side <= 1; side += 2)
    for (int step = -8; step <= 8; ++step) {
      const double n2 = 1.0 + side * 1e-4 + step * 1e-7;
      const float w = (float)std::sqrt(n2 / 2.0);
      const float T[7] = {w, 0.0f, 0.0f, -w, 0.0f, 1.0f, 2.0f};
      defect_line(T);
      const float U[7] = {(float)std::sqrt(n2), 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 2.0f};
      defect_line(U);
    }
  for (float w : {0.0f, 0.5f, 0.99f, 1.01f, 2.0f, 1e20f}) {
    const float T[7] = {w, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    defect_line(T);
  }
  std::printf("pose_rule_check ok\n");
  return 0;
}
