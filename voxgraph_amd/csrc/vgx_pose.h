// The one pose rule: a pose is {qw, qx, qy, qz, tx, ty, tz} in f32.  Rotation is Eigen's _transformVector in the
// association ((v + w uv) + u x uv), uv = 2 (u x v); a rigid transform adds t last; T.inverse() is the conjugate rotation
// and the translation -(q^-1 t), as kindr forms it; a pose is accepted when it is finite and | |q|^2 - 1 | <= 1e-4.
// Every map product is pinned to these bits by a numpy restatement (tests/projected_map_ref.py), so this is the one copy.
// Self-contained: a plain C++ compiler can include it (tests/cpp/pose_rule_check.cpp).
#ifndef VGX_POSE_H_
#define VGX_POSE_H_

#include <cmath>

#ifdef __HIPCC__
#define VGX_POSE_INLINE __forceinline__
#else
#define __host__
#define __device__
#define VGX_POSE_INLINE inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vgx {

__host__ __device__ VGX_POSE_INLINE void quat_rotate(const float q[4], const float v[3], float out[3]) {
  float uv0 = q[2] * v[2] - q[3] * v[1], uv1 = q[3] * v[0] - q[1] * v[2], uv2 = q[1] * v[1] - q[2] * v[0];
  uv0 += uv0;
  uv1 += uv1;
  uv2 += uv2;
  const float c0 = q[2] * uv2 - q[3] * uv1, c1 = q[3] * uv0 - q[1] * uv2, c2 = q[1] * uv1 - q[2] * uv0;
  out[0] = (v[0] + q[0] * uv0) + c0;
  out[1] = (v[1] + q[0] * uv1) + c1;
  out[2] = (v[2] + q[0] * uv2) + c2;
}

__host__ __device__ VGX_POSE_INLINE void rigid_apply(const float q[4], const float t[3], const float v[3], float out[3]) {
  float r[3];
  quat_rotate(q, v, r);
  out[0] = r[0] + t[0];
  out[1] = r[1] + t[1];
  out[2] = r[2] + t[2];
}

// (through rigid_apply with a zero translation, then negated: -(r + 0) is -r but for r = -0, and is what the products
// have always computed)
inline void inverse_pose(const float q[4], const float t[3], float qi[4], float ti[3]) {
  qi[0] = q[0];
  qi[1] = -q[1];
  qi[2] = -q[2];
  qi[3] = -q[3];
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  float r[3];
  rigid_apply(qi, zero, t, r);
  for (int a = 0; a < 3; ++a) ti[a] = -r[a];
}

enum PoseDefect { kPoseOk = 0, kPoseNotFinite, kPoseNotUnit };

// all seven values are looked at for finiteness before the norm is
inline PoseDefect pose_defect(const float T[7]) {
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(T[k])) return kPoseNotFinite;
  const double n2 = (double)T[0] * T[0] + (double)T[1] * T[1] + (double)T[2] * T[2] + (double)T[3] * T[3];
  return std::fabs(n2 - 1.0) > 1e-4 ? kPoseNotUnit : kPoseOk;
}

}  // namespace vgx

#endif  // VGX_POSE_H_
