// REG path: RegistrationCostFunction::Evaluate on gfx950.
//
// Reference: voxgraph/src/backend/constraint/cost_functions/
// registration_cost_function.cpp:58-298 (cited below as RCF:line) and the
// voxblox interpolator / minkindr semantics restated in SURVEY.md Appendix B.
//
// The kernels are HBM/L2-gather bound (88 B per evaluation in the
// materialising f32 form, 52 B in the fused form, ~200 flop): no MFMA.  Per
// residual one thread streams a 20-byte point, finds its base voxel with the
// reference's own f32 floor arithmetic, fetches the 8 trilinear neighbours as
// four 8-byte loads from ONE apron brick (vgx_internal.h) and either stores
// residual + two 1x4 Jacobians or accumulates the 21 unique products of
// [J r]^T [J r].  Floating-point contraction is off so that every floor()
// decision agrees with the CPU restatement bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "vgx_internal.h"

#pragma clang fp contract(off)

namespace vgx {

// ---------------------------------------------------------------------------
// host: per-evaluation pose pack (RCF:69-110 in the reference's f32 arithmetic)
// ---------------------------------------------------------------------------
namespace {
struct YawQuat {
  float w, z;
};

// minkindr RotationQuaternionTemplate<float>::exp for (0,0,psi) [recalled]:
// double internals (Grassia 1998), narrowed to float.
YawQuat yaw_exp(float psi) {
  float nrm = std::sqrt(0.0f * 0.0f + 0.0f * 0.0f + psi * psi);
  double theta = (double)nrm;
  double na = theta < std::pow(2.220446049250313e-16, 0.25)
                  ? 0.5 + (theta * theta) * (1.0 / 48.0)
                  : std::sin(theta * 0.5) / theta;
  double ct = std::cos(theta * 0.5);
  return {(float)ct, (float)((double)psi * na)};
}

// Eigen _transformVector for a yaw-only quaternion (x = y = 0); the dropped
// terms are exact zeros.
void yaw_rotate(YawQuat q, const float v[3], float out[3]) {
  float uv0 = -(q.z * v[1]);
  float uv1 = q.z * v[0];
  uv0 += uv0;
  uv1 += uv1;
  float c0 = -(q.z * uv1);
  float c1 = q.z * uv0;
  out[0] = v[0] + q.w * uv0 + c0;
  out[1] = v[1] + q.w * uv1 + c1;
  out[2] = v[2];
}
}  // namespace

void make_pose_pack(const double ref_pose[4], const double read_pose[4], PosePack* out) {
  std::memset(out, 0, sizeof(*out));
  // RCF:69-88: f64 parameters narrowed into float Vector6, Transformation::exp
  float t_ref[3] = {(float)ref_pose[0], (float)ref_pose[1], (float)ref_pose[2]};
  float t_read[3] = {(float)read_pose[0], (float)read_pose[1], (float)read_pose[2]};
  float yaw_ref = (float)ref_pose[3], yaw_read = (float)read_pose[3];
  YawQuat q_ref = yaw_exp(yaw_ref), q_read = yaw_exp(yaw_read);
  // RCF:109-110: T_mission__reading.inverse() * T_mission__reference
  YawQuat q_inv = {q_read.w, -q_read.z};
  float t_inv[3], rt[3];
  yaw_rotate(q_inv, t_read, t_inv);
  yaw_rotate(q_inv, t_ref, rt);
  out->qw = q_inv.w * q_ref.w - q_inv.z * q_ref.z;
  out->qz = q_inv.w * q_ref.z + q_inv.z * q_ref.w;
  out->tx = -t_inv[0] + rt[0];
  out->ty = -t_inv[1] + rt[1];
  out->tz = -t_inv[2] + rt[2];
  // RCF:91-100
  out->cos_e = std::cos(yaw_read);
  out->sin_e = std::sin(yaw_read);
  out->cos_emo = std::cos(yaw_read - yaw_ref);
  out->sin_emo = std::sin(yaw_read - yaw_ref);
  float dx = t_read[0] - t_ref[0], dy = t_read[1] - t_ref[1];
  out->dxs = dx * out->sin_e;
  out->dxc = dx * out->cos_e;
  out->dys = dy * out->sin_e;
  out->dyc = dy * out->cos_e;
  // lean fused kernel only (the exact kernels keep the reference's association, RCF:225-226)
  out->k1 = out->dxs - out->dyc;
  out->k2 = out->dxc + out->dys;
}

std::vector<Tile> make_tiles(int32_t constraint, int64_t n, int tile_points) {
  std::vector<Tile> tiles;
  for (int64_t s = 0; s < n; s += tile_points) {
    Tile t;
    t.constraint = constraint;
    t.start = s;
    t.count = (int32_t)std::min<int64_t>(tile_points, n - s);
    tiles.push_back(t);
  }
  return tiles;
}

// ---------------------------------------------------------------------------
// device: per-point arithmetic
// ---------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef f32x2 f32x2u __attribute__((aligned(4)));  // 8-byte load, 4-byte aligned
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Pointers read out of descriptor structs are generic; tell the compiler they
// are global memory so it emits global_load_* instead of flat_load_*.
#define VGX_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ const VGX_GLOBAL T* as_global(const T* p) {
  return (const VGX_GLOBAL T*)p;
}

// One axis of Interpolator::setIndexes + getQVector [recalled]: block index,
// base voxel index and fractional offset, all in the reference's f32 steps.
template <int VPS>
__device__ __forceinline__ void locate_axis(float p, const GridDev& g, int& blk, int& vox,
                                            float& delta) {
  blk = (int)floorf(p * g.block_size_inv + 1e-6f);
  float origin = (float)blk * g.block_size;
  int v = (int)floorf((p - origin) * g.voxel_size_inv + 1e-6f);
  v = min(max(v, 0), VPS - 1);
  float centre = origin + ((float)v + 0.5f) * g.voxel_size;
  if (p - centre < 0.0f) {
    v--;
    if (v < 0) {
      blk--;
      v += VPS;
    }
  }
  float origin2 = (float)blk * g.block_size;
  float centre2 = origin2 + ((float)v + 0.5f) * g.voxel_size;
  delta = (p - centre2) * g.voxel_size_inv;
  vox = v;
}

struct PointEval {
  bool ok;             // interp_possible
  double r;            // unscaled residual (RCF:161-166)
  float jo0, jo1, jo2, jo3;  // unscaled d r / d reference pose (RCF:234-236)
  float je3;           // d r / d reading yaw; je0..2 == -jo0..2 (RCF:223-227)
};

template <int VPS, int LAYOUT>
__device__ __forceinline__ void load_neighbours(const float* cell, float d[8]) {
  // neighbour k sits at base + (k>>2 & 1, k>>1 & 1, k & 1)
  if (LAYOUT == 1) {
    // quad brick: {(y,z), (y+1,z), (y,z+1), (y+1,z+1)} of x, then of x + 1
    const f32x4 q0 = *(const VGX_GLOBAL f32x4*)(cell);
    const f32x4 q1 = *(const VGX_GLOBAL f32x4*)(cell + 4);
    d[0] = q0.x; d[2] = q0.y; d[1] = q0.z; d[3] = q0.w;
    d[4] = q1.x; d[6] = q1.y; d[5] = q1.z; d[7] = q1.w;
  } else {
    constexpr int SY = VPS + 1, SZ = (VPS + 1) * (VPS + 1);
    // x is the contiguous axis, so (k, k+4) is one 8-byte load
    f32x2 p0 = *(const VGX_GLOBAL f32x2u*)(cell);
    f32x2 p1 = *(const VGX_GLOBAL f32x2u*)(cell + SZ);
    f32x2 p2 = *(const VGX_GLOBAL f32x2u*)(cell + SY);
    f32x2 p3 = *(const VGX_GLOBAL f32x2u*)(cell + SY + SZ);
    d[0] = p0.x; d[4] = p0.y;
    d[1] = p1.x; d[5] = p1.y;
    d[2] = p2.x; d[6] = p2.y;
    d[3] = p3.x; d[7] = p3.y;
  }
}

// Branch-free two-stage point location + load_neighbours used by the kernels: all
// lanes compute clamped, always-valid addresses, so the block-table loads of every point
// a thread owns issue back to back, then all brick gathers issue back to back (one memory
// round trip each instead of one per point behind divergent branches).  `have` says
// whether the gathered values mean anything.
struct Located {
  int lut_index;   // clamped index into the block table
  int cell_off;    // offset of the base voxel inside a brick
  bool inside;     // base block index within the table's box
  float Dx, Dy, Dz;
};

template <int VPS, int LAYOUT>
__device__ __forceinline__ Located locate_stage1(const GridDev& g, const PosePack& P, float x, float y,
                                                 float z) {
  float uv0 = -(P.qz * y);
  float uv1 = P.qz * x;
  uv0 += uv0;
  uv1 += uv1;
  float c0 = -(P.qz * uv1);
  float c1 = P.qz * uv0;
  float px = (x + P.qw * uv0 + c0) + P.tx;
  float py = (y + P.qw * uv1 + c1) + P.ty;
  float pz = z + P.tz;
  Located L;
  int bx, by, bz, vx, vy, vz;
  locate_axis<VPS>(px, g, bx, vx, L.Dx);
  locate_axis<VPS>(py, g, by, vy, L.Dy);
  locate_axis<VPS>(pz, g, bz, vz, L.Dz);
  bx -= g.lut_min[0];
  by -= g.lut_min[1];
  bz -= g.lut_min[2];
  L.inside = (unsigned)bx < (unsigned)g.lut_dim[0] && (unsigned)by < (unsigned)g.lut_dim[1] &&
             (unsigned)bz < (unsigned)g.lut_dim[2];
  int cx = min(max(bx, 0), g.lut_dim[0] - 1), cy = min(max(by, 0), g.lut_dim[1] - 1),
      cz = min(max(bz, 0), g.lut_dim[2] - 1);
  L.lut_index = cx + g.lut_dim[0] * (cy + g.lut_dim[1] * cz);
  L.cell_off = BrickLayout<VPS, LAYOUT>::anchor(vx, vy, vz);
  return L;
}

// The interpolated distance in the reference's own association: c = interp_table_ * distances^T
// (registration_cost_function.h:73-81), q_vector (Interpolator::getQVector), their product (RCF:158-159);
// no contraction (this file compiles with fp contract off).  Shared by the exact kernel and the fused
// kernel: the residual d_ref - value amplifies a one-ulp difference in the value by |value / residual|,
// so the fused kernel must not have its own association here (see eval_point_lean).
__device__ __forceinline__ float interpolated_value(const float d[8], float Dx, float Dy, float Dz, float& c0,
                                                    float& c1, float& c2, float& c3, float& c4, float& c5,
                                                    float& c6, float& c7) {
  c0 = d[0];
  c1 = -d[0] + d[4];
  c2 = -d[0] + d[2];
  c3 = -d[0] + d[1];
  c4 = ((d[0] - d[2]) - d[4]) + d[6];
  c5 = ((d[0] - d[1]) - d[2]) + d[3];
  c6 = ((d[0] - d[1]) - d[4]) + d[5];
  c7 = (((((( -d[0] + d[1]) + d[2]) - d[3]) + d[4]) - d[5]) - d[6]) + d[7];
  const float q4 = Dx * Dy, q5 = Dy * Dz, q6 = Dz * Dx, q7 = Dx * Dy * Dz;
  return ((((((c0 + Dx * c1) + Dy * c2) + Dz * c3) + q4 * c4) + q5 * c5) + q6 * c6) + q7 * c7;
}

__device__ __forceinline__ PointEval eval_point(const float d[8], bool have, float Dx, float Dy,
                                                float Dz, float inv_f, const PosePack& P, float xi,
                                                float yi, float d_ref, float w,
                                                double no_corr_cost, bool want_jac) {
  PointEval e;
  // every neighbour valid <=> no NaN among the 8 (apron-brick encoding)
  float s = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
  bool ok = have && (s == s);
  e.ok = ok;
  e.jo0 = e.jo1 = e.jo2 = e.jo3 = e.je3 = 0.0f;
  if (!ok) {
    e.r = (double)w * no_corr_cost;  // RCF:165-166
    return e;
  }
  // c = interp_table_ * distances^T (registration_cost_function.h:73-81)
  float c0, c1, c2, c3, c4, c5, c6, c7;
  const float dot = interpolated_value(d, Dx, Dy, Dz, c0, c1, c2, c3, c4, c5, c6, c7);
  e.r = ((double)d_ref - (double)dot) * (double)w;  // RCF:161-163
  if (!want_jac) return e;
  // RCF:183-202: doubles rounded into a float matrix
  double inv = (double)inv_f, dx = (double)Dx, dy = (double)Dy, dz = (double)Dz;
  float iDx = (float)(inv * dx), iDy = (float)(inv * dy), iDz = (float)(inv * dz);
  float iDyDz = (float)(inv * dy * dz), iDxDz = (float)(inv * dx * dz), iDxDy = (float)(inv * dx * dy);
  // RCF:204-205
  float g0 = ((c1 * inv_f + c4 * iDy) + c6 * iDz) + c7 * iDyDz;
  float g1 = ((c2 * inv_f + c4 * iDx) + c5 * iDz) + c7 * iDxDz;
  float g2 = ((c3 * inv_f + c5 * iDy) + c6 * iDx) + c7 * iDxDy;
  // RCF:214-239
  float h0 = -w * g0, h1 = -w * g1, h2 = -w * g2;
  float mo3 = xi * P.sin_emo - yi * P.cos_emo;
  float mo7 = xi * P.cos_emo + yi * P.sin_emo;
  float me3 = ((-xi * P.sin_emo + yi * P.cos_emo) + P.dxs) - P.dyc;
  float me7 = ((-xi * P.cos_emo - yi * P.sin_emo) + P.dxc) + P.dys;
  e.jo0 = h0 * P.cos_e + h1 * -P.sin_e;
  e.jo1 = h0 * P.sin_e + h1 * P.cos_e;
  e.jo2 = h2;
  e.jo3 = h0 * mo3 + h1 * mo7;
  e.je3 = h0 * me3 + h1 * me7;
  return e;
}

template <typename T>
struct Out4;
template <>
struct Out4<float> {
  using type = float4;
  static __device__ __forceinline__ float4 make(double a, double b, double c, double d) {
    return make_float4((float)a, (float)b, (float)c, (float)d);
  }
};
template <>
struct Out4<double> {
  using type = double4;
  static __device__ __forceinline__ double4 make(double a, double b, double c, double d) {
    return make_double4(a, b, c, d);
  }
};

// Tiles run in launch order.  An XCD-aware order (workgroup b runs on XCD b % 8, so each XCD could be
// handed one contiguous range of tiles to keep neighbouring bricks in one L2) MEASURED SLOWER here
// (5.24-5.55 ms vs 5.03-5.31 ms for the materialising kernel, 2.66 vs 2.54 ms fused): the kernels are
// HBM-stream bound, the gathers already hit in L2/MALL, and eight XCDs streaming eight distant address
// ranges is worse for the memory system than one interleaved front.

// True when no point inside the sphere (centre in the reference frame) can have a
// correspondence in grid g under pose pack P: the base block of p' is the block of p'
// or its -1 neighbour, so p' must lie in [lut_min * bs, (lut_min + lut_dim + 1) * bs);
// one voxel of slack covers the f32 rounding of the transformed centre.
__host__ __device__ __forceinline__ bool chunk_outside(const GridDev& g, const PosePack& P, float4 sph) {
  float uv0 = -(P.qz * sph.y), uv1 = P.qz * sph.x;
  uv0 += uv0;
  uv1 += uv1;
  float cx = (sph.x + P.qw * uv0 - P.qz * uv1) + P.tx;
  float cy = (sph.y + P.qw * uv1 + P.qz * uv0) + P.ty;
  float cz = sph.z + P.tz;
  float r = sph.w + g.voxel_size;
  float lox = (float)g.lut_min[0] * g.block_size, hix = (float)(g.lut_min[0] + g.lut_dim[0] + 1) * g.block_size;
  float loy = (float)g.lut_min[1] * g.block_size, hiy = (float)(g.lut_min[1] + g.lut_dim[1] + 1) * g.block_size;
  float loz = (float)g.lut_min[2] * g.block_size, hiz = (float)(g.lut_min[2] + g.lut_dim[2] + 1) * g.block_size;
  return cx + r < lox || cx - r > hix || cy + r < loy || cy - r > hiy || cz + r < loz || cz - r > hiz;
}

// ---------------------------------------------------------------------------
// kernel 1: materialise residuals + Jacobians (88 B / evaluation as f32)
// ---------------------------------------------------------------------------
// Output rows are written once and never re-read by this kernel: the f32 stores carry the
// non-temporal hint so the 36 B/row write stream does not evict the bricks and block tables the
// gathers re-use from L2 (measured 6.08 -> 5.40 ms).  Point loads stay plain.
template <typename T>
__device__ __forceinline__ void store_out(T* p, T v) {
  __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ void store_out4(float4* p, float4 v) {
  f32x4 x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<f32x4*>(p));
}
__device__ __forceinline__ void store_out4(double4* p, double4 v) {
  *p = v;  // drop-in f64 path: followed by a D2H copy, keep it cacheable
}

// WeightedSampler::getRandomItem (weighted_sampler_inl.h:18-28) for residual i, from the two raw
// std::mt19937 outputs the host drew for it.  std::uniform_real_distribution<double>(0, 1) is
// libstdc++'s generate_canonical<double, 53>: (first + second * 2^32) / 2^64 with the first output
// as the LOW part, the sum rounded once to double, and 1.0 mapped to the largest double below it.
// Every operation is an IEEE f64 operation or an exact scaling, so this is the host's arithmetic.
// Stages of the draw, split so that a caller can run several draws in lock step (every stage is one
// dependent memory access; reg_draw_kernel keeps four draws per lane in flight):
struct DrawState {
  double target;
  int64_t first, len;
};
// What bounds the draw is the number of SCATTERED lane addresses its loads present to the CU's address /
// tag pipeline (one per clock: measured 52 G draws/s with 6 scattered 4- and 8-byte loads per draw, whatever
// the occupancy and the HBM traffic), so neighbouring words are fetched by ONE wider load each: the bucket
// pair {lut[k], lut[k + 1]} as 8 bytes, the cumulative weights as 16-byte pairs (4- / 8-byte aligned
// addresses: gfx950 global loads need dword alignment only).
typedef uint32_t u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));
typedef int32_t i32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef double f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

__device__ __forceinline__ double draw_uniform(const ConstraintDev& C, int64_t i) {
  // (2 words per residual from an even offset of a 256-byte aligned stream: 8-byte aligned)
  const u32x2_a8 raw = *reinterpret_cast<const VGX_GLOBAL u32x2_a8*>(as_global(C.sample_raw) + 2 * i);
  const double lo = (double)raw.x;
  const double hi = (double)raw.y;
  // ... / 2^64 as a multiplication: an exact scaling either way
  double u = (lo + hi * 4294967296.0) * 0x1p-64;
  if (u >= 1.0) u = 0x1.fffffffffffffp-1;  // std::nextafter(1.0, 0.0)
  return u;
}
__device__ __forceinline__ DrawState draw_bucket(const ConstraintDev& C, double u, double total) {
  DrawState d;
  d.target = u * total;  // random_number * cumulative.back()
  d.first = 0;
  d.len = C.n_points;    // std::upper_bound over everything
  if (C.search_lut) {
    // u in [k / K, (k + 1) / K)  =>  the bound lies in [lut[k], lut[k + 1]] (monotonicity of u * total
    // and of upper_bound); searching that sub-range returns exactly what the full search returns.
    // K is a power of two >= n: u * K is exact, the range holds about one element.
    const int k = (int)(u * (double)C.search_buckets);
    const i32x2_a4 b = *reinterpret_cast<const VGX_GLOBAL i32x2_a4*>(as_global(C.search_lut) + k);
    d.first = b.x;
    d.len = b.y - b.x;
  }
  return d;
}
__device__ __forceinline__ int32_t draw_finish(const ConstraintDev& C, DrawState d) {
  const double* cum = C.cumulative;
  if (d.len <= 4) {
    // the elements <= target are a prefix of the sorted range: count them.  cum[first .. first + 3] in two
    // 16-byte loads (the table carries 3 entries of padding; entries beyond the range are not used); a
    // wavefront whose ranges all hold at most two elements -- the usual case, the table has >= n buckets --
    // issues only the first
    const int64_t at = d.first < C.n_points ? d.first : C.n_points - 1;  // (first == n: empty range at the end)
    const f64x2_a8 c01 = *reinterpret_cast<const VGX_GLOBAL f64x2_a8*>(as_global(cum) + at);
    int64_t below = (int64_t)((d.len > 0) & !(d.target < c01.x)) + (int64_t)((d.len > 1) & !(d.target < c01.y));
    if (__builtin_amdgcn_ballot_w64(d.len > 2) != 0ull) {
      const f64x2_a8 c23 = *reinterpret_cast<const VGX_GLOBAL f64x2_a8*>(as_global(cum) + at + 2);
      below += (int64_t)((d.len > 2) & !(d.target < c23.x)) + (int64_t)((d.len > 3) & !(d.target < c23.y));
    }
    d.first += below;
    d.len = 0;
  }
  while (d.len > 0) {
    const int64_t half = d.len >> 1;
    if (!(d.target < as_global(cum)[d.first + half])) {
      d.first += half + 1;
      d.len -= half + 1;
    } else {
      d.len = half;
    }
  }
  if (d.first >= C.n_points) d.first = C.n_points - 1;
  return C.inv_order ? as_global(C.inv_order)[d.first] : (int32_t)d.first;
}
__device__ __forceinline__ int32_t weighted_draw(const ConstraintDev& C, int64_t i) {
  const double total = as_global(C.cumulative)[C.n_points - 1];
  return draw_finish(C, draw_bucket(C, draw_uniform(C, i), total));
}

// The batch draws once per evaluation, ahead of the pass that uses the points: a thin kernel (every
// lane four independent chains raw -> bucket table -> cumulative weights, launched so that the draws of
// one point set run on one XCD with its tables in that L2: make_draw_order) hides the dependent loads
// far better than the evaluation kernels' 80-100 VGPR waves did, and both passes read the 4-byte
// result coalesced.  Shipped configuration (19.3 M draws): 2.49 ms fused kernel with the draw inside ->
// 0.38 ms draw kernel + 0.97 ms fused kernel (2.90 -> 1.63 ms per solver evaluation with the faster
// mt_generate_kernel).
// Round 4: the draws come to the evaluation kernels as POINTS {x, y, z, d} (16 B per row, coalesced), so those
// kernels stream their points like the all-points passes do.  Two kernels, both PERSISTENT and XCD-aware:
// workgroup b serves XCD b % 8 (the dispatcher deals workgroups round the XCDs) and walks that XCD's share
// of the tile sequence (make_draw_order: one point set after the other) together with the XCD's other
// workgroups, `wgs_per_xcd` tiles at a time -- about ONE point set is in flight per XCD, so
//   reg_draw_kernel           finds the set's cumulative weights (8 B x n) and bucket table in that L2
//                             (2.4 MB for a 256^3 submap's isosurface points; a plain launch keeps ~3 sets
//                             in flight per XCD and thrashes: 3.1 GB of HBM reads per 19.3 M draws measured),
//   reg_gather_points_kernel  finds the set's points (16 B x n, 2.6 MB) there: every 128-byte line of it is
//                             wanted by ~5 of the ~12 constraints that draw from the set.
// Together the tables would not fit one 4 MB L2: hence two passes with a 4-byte index in between.
constexpr int kDrawWgsPerXcdDefault = 96;

__global__ __launch_bounds__(256) void reg_draw_kernel(const ConstraintDev* __restrict__ cons,
                                                      const Tile* __restrict__ tiles, int n_tiles, int wgs_per_xcd,
                                                      int32_t* __restrict__ drawn_idx) {
  const int xcd = blockIdx.x & 7, local_wg = blockIdx.x >> 3;
  for (int q = local_wg;; q += wgs_per_xcd) {
    const int t = q * 8 + xcd;
    if (t >= n_tiles) break;
    const Tile tile = tiles[t];
    const ConstraintDev& C = cons[tile.constraint];
    if (!C.sample_raw) continue;
    const double total = as_global(C.cumulative)[C.n_points - 1];
    constexpr int D = kTilePoints / 256;
    double u[D];
    DrawState d[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int local = j * 256 + (int)threadIdx.x;
      u[j] = draw_uniform(C, tile.start + (local < tile.count ? local : 0));
    }
#pragma unroll
    for (int j = 0; j < D; ++j) d[j] = draw_bucket(C, u[j], total);
    int32_t s[D];
#pragma unroll
    for (int j = 0; j < D; ++j) s[j] = draw_finish(C, d[j]);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int local = j * 256 + (int)threadIdx.x;
      if (local < tile.count) drawn_idx[C.row0 + tile.start + local] = s[j];
    }
  }
}

__global__ __launch_bounds__(256) void reg_gather_points_kernel(const ConstraintDev* __restrict__ cons,
                                                               const Tile* __restrict__ tiles, int n_tiles,
                                                               int wgs_per_xcd, const int32_t* __restrict__ drawn_idx,
                                                               float4* __restrict__ drawn) {
  const int xcd = blockIdx.x & 7, local_wg = blockIdx.x >> 3;
  for (int q = local_wg;; q += wgs_per_xcd) {
    const int t = q * 8 + xcd;
    if (t >= n_tiles) break;
    const Tile tile = tiles[t];
    const ConstraintDev& C = cons[tile.constraint];
    if (!C.sample_raw) continue;
    constexpr int D = kTilePoints / 256;
    int32_t s[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int local = j * 256 + (int)threadIdx.x;
      s[j] = __builtin_nontemporal_load(drawn_idx + C.row0 + tile.start + (local < tile.count ? local : 0));
    }
    f32x4 p[D];
#pragma unroll
    for (int j = 0; j < D; ++j) p[j] = as_global(reinterpret_cast<const f32x4*>(C.xyzd))[s[j]];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int local = j * 256 + (int)threadIdx.x;
      if (local < tile.count)
        __builtin_nontemporal_store(p[j], reinterpret_cast<f32x4*>(drawn) + C.row0 + tile.start + local);
    }
  }
}

// Which residual of its tile a thread takes in slot j.  With shift 0 it is j * kBlockThreads + threadIdx.x.  The rows
// pass rotates the assignment by shift = (first row of the tile) & 63, so that the 64 rows one wavefront stores with one
// instruction begin on a multiple of 64 rows of the output arrays -- whole 256-byte (residuals) and 1 KiB (Jacobian)
// spans, where an unrotated wavefront shares a partly written sector with its neighbour at both ends.  The first
// span of a tile is then `shift` rows short: those lanes wrap to the last `shift` residuals of a whole tile.  Every
// residual of the tile is still taken by exactly one (thread, slot); a slot is active iff its residual is < the count.
template <int PPT>
__device__ __forceinline__ int tile_local(int j, int shift) {
  static_assert(((PPT * kBlockThreads) & (PPT * kBlockThreads - 1)) == 0, "the rotation wraps with a mask");
  return (j * kBlockThreads + (int)threadIdx.x - shift) & (PPT * kBlockThreads - 1);
}

// The PPT points (and weights) of one thread of a materialising tile: residual tile_local(j, shift) of the
// `count` that start at `start`; lanes past the end load residual `start` and drop it later.  A sampling constraint
// (RCF:113-122) uses the batch's precomputed draw, or (one-constraint drop-in launch) draws here, with weight 1.
// Which of the three sources it is, is decided ONCE, around whole loops: with the test inside the per-point loop the
// compiler branches round every point's loads and waits vmcnt(0) at each merge, so point j + 1 was requested only when
// point j had arrived -- PPT dependent round trips where one is needed (profiles/points_load_chain.txt).  As written
// every load of a path is issued before the first wait.
template <int PPT>
__device__ __forceinline__ void load_tile_points(const ConstraintDev& C, int64_t start, int count, int shift,
                                                 f32x4 pt[PPT], float w[PPT]) {
  int64_t i[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int local = tile_local<PPT>(j, shift);
    i[j] = start + (local < count ? local : 0);
  }
  if (C.sample_raw == nullptr) {
#pragma unroll
    for (int j = 0; j < PPT; ++j) pt[j] = as_global(reinterpret_cast<const f32x4*>(C.xyzd))[i[j]];
#pragma unroll
    for (int j = 0; j < PPT; ++j) w[j] = as_global(C.weight)[i[j]];
    return;
  }
  if (C.sample_pts) {
#pragma unroll
    for (int j = 0; j < PPT; ++j) pt[j] = as_global(reinterpret_cast<const f32x4*>(C.sample_pts))[C.row0 + i[j]];
  } else {
#pragma unroll
    for (int j = 0; j < PPT; ++j) pt[j] = as_global(reinterpret_cast<const f32x4*>(C.xyzd))[weighted_draw(C, i[j])];
  }
#pragma unroll
  for (int j = 0; j < PPT; ++j) w[j] = 1.0f;  // RCF:121
}


// Chunk culling of the materialising pass (see reg_eval_points_body)
__device__ __forceinline__ bool tile_cullable(const ConstraintDev& C) {
  return C.no_corr_cost == 0.0 && C.sample_raw == nullptr && C.chunk_bounds != nullptr;
}
template <int PPT>
__device__ __forceinline__ bool tile_outside(const ConstraintDev& C, const PosePack& P, const Tile& tile) {
  const long long chunk0 = tile.start / kChunkPoints;  // tiles start on chunk boundaries
  bool any_live = false;
#pragma unroll
  for (int q = 0; q < (kBlockThreads * PPT) / kChunkPoints; ++q)
    if (q * kChunkPoints < tile.count) any_live |= !chunk_outside(C.grid, P, C.chunk_bounds[chunk0 + q]);
  return !any_live;
}
// one thread per tile of the batched launch, in launch order.  The verdicts leave as one bit per tile, a wavefront's 64
// in one 64-bit ballot (bit t & 31 of 32-bit word t >> 5): reg_eval_points_kernel reads its tile's word at a uniform
// index, which a 32-bit word lets the compiler do on the scalar path, in the same clause as the tile descriptor (a
// byte load goes through the vector path: one more round trip in front of every workgroup's first descriptor load).
template <int PPT>
__global__ __launch_bounds__(256) void reg_points_tile_dead_kernel(const ConstraintDev* __restrict__ cons,
                                                                  const PosePack* __restrict__ packs,
                                                                  const Tile* __restrict__ tiles, int n_tiles,
                                                                  unsigned long long* __restrict__ dead) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  bool verdict = false;
  if (t < n_tiles) {
    const Tile tile = tiles[t];
    const ConstraintDev& C = cons[tile.constraint];
    verdict = tile_cullable(C) && tile_outside<PPT>(C, packs[tile.constraint], tile);
  }
  const unsigned long long mask = __ballot(verdict);
  if ((threadIdx.x & 63) == 0 && t < n_tiles) dead[t >> 6] = mask;  // t: the wavefront's first tile, a multiple of 64
}
// bytes of the verdict words of n_tiles tiles
static inline size_t tile_dead_bytes(size_t n_tiles) { return ((n_tiles + 63) / 64) * sizeof(unsigned long long); }

template <int VPS, int LAYOUT, typename OUT, int PPT>
__device__ __forceinline__ void reg_eval_points_body(
    const ConstraintDev& C, const PosePack& P, const Tile& tile, int dead_hint, int shift, OUT* __restrict__ residuals,
    typename Out4<OUT>::type* __restrict__ jac_ref, typename Out4<OUT>::type* __restrict__ jac_read) {
  const GridDev g = C.grid;
  const bool want_jac =(jac_ref != nullptr) | (jac_read != nullptr);
  // Chunk culling, as in the fused pass: when the bounding spheres of the tile's 512-point chunks all
  // map outside the reading submap's block box, none of its points finds a block (RCF:165-166), so
  // with no_correspondence_cost == 0 its rows are zeros whatever the points are: they are written
  // without reading the points at all (36 B per evaluation instead of 56).  Tiles start on chunk
  // boundaries; the test is uniform over the workgroup.  A tile with one chunk in and one out takes
  // the straight-line path below for both (its code stays free of per-chunk branches).
  // The batched launch gets the verdict from reg_points_tile_dead_kernel (dead_hint 0 / 1, loaded
  // together with the tile descriptor: the bounds test adds no dependent memory latency in front of
  // the point loads -- in-kernel it cost 5-7 % on a workload with nothing to cull); the one-constraint
  // drop-in launch decides here (dead_hint < 0).
  {
    bool any_live = dead_hint == 0;
    if (dead_hint < 0) {
      any_live = true;
      if (tile_cullable(C)) any_live = !tile_outside<PPT>(C, P, tile);
    }
    if (!any_live) {
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        int local = tile_local<PPT>(j, shift);
        if (local >= tile.count) continue;
        int64_t row = C.row0 + tile.start + local;
        store_out(&residuals[row], (OUT)0);  // r = w * 0, Jacobians zero (RCF:165-170)
        if (jac_ref) store_out4(&jac_ref[row], Out4<OUT>::make(0.0, 0.0, 0.0, 0.0));
        if (jac_read) store_out4(&jac_read[row], Out4<OUT>::make(0.0, 0.0, 0.0, 0.0));
      }
      return;
    }
  }

  f32x4 pt[PPT];
  float w[PPT];
  const float* cell[PPT];
  float Dx[PPT], Dy[PPT], Dz[PPT];
  float d[PPT][8];
  load_tile_points<PPT>(C, tile.start, tile.count, shift, pt, w);
  // stage 1: exact base voxel of every point (registers only)
  Located loc[PPT];
  bool have[PPT];
  const bool grid_empty = g.bricks == nullptr;  // reading submap without blocks
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    loc[j] = locate_stage1<VPS, LAYOUT>(g, P, pt[j].x, pt[j].y, pt[j].z);
    Dx[j] = loc[j].Dx;
    Dy[j] = loc[j].Dy;
    Dz[j] = loc[j].Dz;
    have[j] = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[j][k] = 0.0f;
    cell[j] = nullptr;
  }
  if (!grid_empty) {
    // stage 2: all block-table loads, then all brick gathers
    int slot[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) slot[j] = as_global(g.lut)[loc[j].lut_index];
    constexpr int CELLS = BrickLayout<VPS, LAYOUT>::cells;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      have[j] = loc[j].inside && slot[j] >= 0;
      cell[j] = g.bricks + (size_t)(have[j] ? slot[j] : 0) * CELLS + loc[j].cell_off;
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) load_neighbours<VPS, LAYOUT>(cell[j], d[j]);
  }
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    int local = tile_local<PPT>(j, shift);
    if (local >= tile.count) continue;
    PointEval e = eval_point(d[j], have[j], Dx[j], Dy[j], Dz[j], g.voxel_size_inv, P,
                             pt[j].x, pt[j].y, pt[j].w, w[j], C.no_corr_cost, want_jac);
    int64_t row = C.row0 + tile.start + local;
    const double f = C.factor;  // RCF:274-291
    store_out(&residuals[row], (OUT)(e.r * f));
    if (jac_ref)
      store_out4(&jac_ref[row], Out4<OUT>::make((double)e.jo0 * f, (double)e.jo1 * f,
                                                (double)e.jo2 * f, (double)e.jo3 * f));
    if (jac_read)
      store_out4(&jac_read[row], Out4<OUT>::make((double)-e.jo0 * f, (double)-e.jo1 * f,
                                                 (double)-e.jo2 * f, (double)e.je3 * f));
  }
}

// batched form: descriptors, pose packs and tiles live in device memory
template <int VPS, int LAYOUT, typename OUT, int PPT>
__global__ __launch_bounds__(kBlockThreads) void reg_eval_points_kernel(
    const ConstraintDev* __restrict__ cons, const PosePack* __restrict__ packs,
    const Tile* __restrict__ tiles, const uint32_t* __restrict__ tile_dead, int n_tiles,
    OUT* __restrict__ residuals, typename Out4<OUT>::type* __restrict__ jac_ref,
    typename Out4<OUT>::type* __restrict__ jac_read, int blocked, int shift_mask) {
  const int t = blockIdx.x;
  if (t >= n_tiles) return;
  const Tile tile = tiles[t];
  const int dead = (int)((tile_dead[t >> 5] >> (t & 31)) & 1u);  // reg_points_tile_dead_kernel's bit: a scalar load
  const ConstraintDev& C = cons[tile.constraint];
  if (blocked) {
    // ONE output stream (vgx_reg_batch_evaluate_points_blocked): `residuals` is the base of an array of tile blocks,
    // block = [r x kTilePoints][jac_ref x kTilePoints][jac_read x kTilePoints], one per tile of every constraint padded to
    // whole tiles.  The three pointers are re-based so that the body's [row0 + start + local] lands inside this tile's block.
    using O4 = typename Out4<OUT>::type;
    constexpr long long kBlockBytes = (long long)(PPT * kBlockThreads) * (long long)(sizeof(OUT) + 2 * sizeof(O4));
    const long long first = C.row0 + tile.start;
    char* blk = reinterpret_cast<char*>(residuals) + ((C.prow0 + tile.start) / (PPT * kBlockThreads)) * kBlockBytes;
    OUT* r_t = reinterpret_cast<OUT*>(blk) - first;
    O4* jr_t = reinterpret_cast<O4*>(blk + (long long)(PPT * kBlockThreads) * (long long)sizeof(OUT)) - first;
    O4* je_t = reinterpret_cast<O4*>(blk + (long long)(PPT * kBlockThreads) * (long long)(sizeof(OUT) + sizeof(O4))) - first;
    reg_eval_points_body<VPS, LAYOUT, OUT, PPT>(C, packs[tile.constraint], tile, dead, /*shift=*/0, r_t, jr_t, je_t);
    return;
  }
  // a constraint's first row is the sum of the counts before it: anything modulo 64 (tile.start is a multiple of the tile).
  // shift_mask is 63, or 0 where the launch keeps its point loads on their lines instead (launch_points)
  const int shift = (int)((C.row0 + tile.start) & shift_mask);
  reg_eval_points_body<VPS, LAYOUT, OUT, PPT>(C, packs[tile.constraint], tile, dead, shift, residuals, jac_ref, jac_read);
}

// drop-in form (one constraint per Evaluate): descriptor and pose pack travel as kernel
// arguments and tiles are implicit, so an Evaluate needs no host->device copy at all
template <int VPS, int LAYOUT, typename OUT, int PPT>
__global__ __launch_bounds__(kBlockThreads) void reg_eval_points_single_kernel(
    ConstraintDev C, PosePack P, int n_tiles, OUT* __restrict__ residuals,
    typename Out4<OUT>::type* __restrict__ jac_ref, typename Out4<OUT>::type* __restrict__ jac_read) {
  const int t = blockIdx.x;
  if (t >= n_tiles) return;
  Tile tile;
  tile.constraint = 0;
  tile.start = (int64_t)t * (kBlockThreads * PPT);
  int64_t left = C.n - tile.start;
  tile.count = (int32_t)(left < kBlockThreads * PPT ? left : kBlockThreads * PPT);
  reg_eval_points_body<VPS, LAYOUT, OUT, PPT>(C, P, tile, /*dead_hint=*/-1, /*shift=*/0, residuals, jac_ref, jac_read);
}

// ---------------------------------------------------------------------------
// kernel 1v: the cost-function visuals of one constraint (vgx_reg_evaluate_visuals)
// ---------------------------------------------------------------------------
// The visuals instantiation of the drop-in materialising pass: same tiles, same point loads (load_tile_points: the same
// draws from the same engine outputs), same locate_stage1 / load_neighbours / eval_point, so r_u and j below are the
// values the rows kernel scales.  What it writes per row (rules: include/voxgraph_amd.h, "Cost-function visuals"):
//   cloud    32 B  pcl::PointXYZI {p_m.x, p_m.y, p_m.z, 1.0f | f32(f64(f32(r_u)) * factor), 0, 0, 0}: two 16-byte stores
//   arrows   48 B  {o, t} f64, o = f64(p_m), t = f64(j) * (factor * 0.05) + o: three 16-byte stores           (GRAD)
//   origins  24 B  o: a tile's origins are one contiguous run that starts 16-byte aligned (kTilePoints is even), so
//                  they are staged in LDS and leave as 16-byte stores, thread k the pair k, k + 256, ..          (GRAD)
// No dead-tile shortcut: a tile outside the reading grid still needs every point's p_m, and its intensity is
// f32(f64(f32(w * no_correspondence_cost)) * factor).
struct VisualsPose {
  float qw, qz;      // T_mission__reading: minkindr exp of (x, y, z, 0, 0, yaw) in f32 (RCF:80-88)
  float tx, ty, tz;
};

template <int VPS, int LAYOUT, int PPT, bool GRAD>
__global__ __launch_bounds__(kBlockThreads) void reg_visuals_single_kernel(ConstraintDev C, PosePack P, VisualsPose M,
                                                                           int n_tiles, f32x4* __restrict__ cloud,
                                                                           double* __restrict__ arrows,
                                                                           double* __restrict__ origins) {
  __shared__ double s_origin[GRAD ? 3 * kBlockThreads * PPT : 1];
  const int t = blockIdx.x;
  if (t >= n_tiles) return;
  const int64_t start = (int64_t)t * (kBlockThreads * PPT);
  const int64_t left = C.n - start;
  const int count = (int)(left < kBlockThreads * PPT ? left : kBlockThreads * PPT);
  const GridDev g = C.grid;

  f32x4 pt[PPT];
  float w[PPT];
  const float* cell[PPT];
  float d[PPT][8];
  load_tile_points<PPT>(C, start, count, /*shift=*/0, pt, w);
  Located loc[PPT];
  bool have[PPT];
  const bool grid_empty = g.bricks == nullptr;  // reading submap without blocks
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    loc[j] = locate_stage1<VPS, LAYOUT>(g, P, pt[j].x, pt[j].y, pt[j].z);
    have[j] = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[j][k] = 0.0f;
    cell[j] = nullptr;
  }
  if (!grid_empty) {
    int slot[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) slot[j] = as_global(g.lut)[loc[j].lut_index];
    constexpr int CELLS = BrickLayout<VPS, LAYOUT>::cells;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      have[j] = loc[j].inside && slot[j] >= 0;
      cell[j] = g.bricks + (size_t)(have[j] ? slot[j] : 0) * CELLS + loc[j].cell_off;
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) load_neighbours<VPS, LAYOUT>(cell[j], d[j]);
  }
  const double f = C.factor;
  const double arrow_scale = __dmul_rn(f, 0.05);  // CFV:82-84: factor * 0.05 first
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    int local = j * kBlockThreads + (int)threadIdx.x;
    if (local >= count) continue;
    PointEval e = eval_point(d[j], have[j], loc[j].Dx, loc[j].Dy, loc[j].Dz, g.voxel_size_inv, P, pt[j].x, pt[j].y,
                             pt[j].w, w[j], C.no_corr_cost, GRAD);
    // p_read = T_reading__reference * p_ref: locate_stage1's own steps (RCF:128-129)
    const float x = pt[j].x, y = pt[j].y, z = pt[j].z;
    float uv0 = -(P.qz * y);
    float uv1 = P.qz * x;
    uv0 += uv0;
    uv1 += uv1;
    float c0 = -(P.qz * uv1);
    float c1 = P.qz * uv0;
    const float px = (x + P.qw * uv0 + c0) + P.tx;
    const float py = (y + P.qw * uv1 + c1) + P.ty;
    const float pz = z + P.tz;
    // p_m = T_mission__reading * p_read (RCF:172-173, 247-248): the same point transform
    uv0 = -(M.qz * py);
    uv1 = M.qz * px;
    uv0 += uv0;
    uv1 += uv1;
    c0 = -(M.qz * uv1);
    c1 = M.qz * uv0;
    const float mx = (px + M.qw * uv0 + c0) + M.tx;
    const float my = (py + M.qw * uv1 + c1) + M.ty;
    const float mz = pz + M.tz;
    const int64_t row = start + local;
    if (cloud) {
      // CFV:49 narrows the unscaled residual, CFV:75 multiplies float by double in f64 and rounds once
      const float intensity = (float)__dmul_rn((double)(float)e.r, f);
      const f32x4 lo = {mx, my, mz, 1.0f}, hi = {intensity, 0.0f, 0.0f, 0.0f};
      cloud[2 * row] = lo;
      cloud[2 * row + 1] = hi;
    }
    if (GRAD) {
      const double ox = (double)mx, oy = (double)my, oz = (double)mz;
      // j = pResidual_pParamRead.head<3>() (RCF:249): je0..2 == -jo0..2
      const double tx = __dadd_rn(__dmul_rn((double)-e.jo0, arrow_scale), ox);
      const double ty = __dadd_rn(__dmul_rn((double)-e.jo1, arrow_scale), oy);
      const double tz = __dadd_rn(__dmul_rn((double)-e.jo2, arrow_scale), oz);
      double2* a = reinterpret_cast<double2*>(arrows + 6 * row);
      a[0] = make_double2(ox, oy);
      a[1] = make_double2(oz, tx);
      a[2] = make_double2(ty, tz);
      s_origin[3 * local] = ox;
      s_origin[3 * local + 1] = oy;
      s_origin[3 * local + 2] = oz;
    }
  }
  if (GRAD) {
    __syncthreads();
    double* out = origins + 3 * start;  // 24 * start bytes: start is a multiple of kBlockThreads * PPT
    const int total = 3 * count, pairs = total / 2;
    for (int k = (int)threadIdx.x; k < pairs; k += kBlockThreads)
      reinterpret_cast<double2*>(out)[k] = make_double2(s_origin[2 * k], s_origin[2 * k + 1]);
    if ((total & 1) && threadIdx.x == 0) out[total - 1] = s_origin[total - 1];  // (an odd tail tile: its last double alone)
  }
}

// ---------------------------------------------------------------------------
// kernel 2: fused normal equations (52 B / evaluation, no per-point output)
// ---------------------------------------------------------------------------
// u = (jo0, jo1, jo2, jo3, je3, r): [J r]^T [J r] (9x9) is a signed
// re-arrangement of the 21 unique products of u because je0..2 == -jo0..2.
constexpr int kReduceIters = 10;  // a fused-pass tile of a large constraint = kTilePoints * kReduceIters residuals (round 4: 20)
// Fused-kernel shape: 2 points per thread, f32 accumulators, 6 waves per SIMD.  Measured on config 3 as
// waves / points per thread / accumulator: 4/2/f64 2.17 ms, 4/2/f32 1.79, 5/2/f32 1.80, 6/2/f32 1.76,
// 6/1/f32 2.07, 8/1/f32 1.95 (the round-1 kernel -- reference operation order, f64 accumulators,
// 124 VGPRs -- 2.23 ms).
constexpr int kLeanPointsPerThread = 2;
constexpr int kLeanWaves = 6;
// a wavefront none of whose points found a reading block skips its gathers and products
constexpr bool kBallotSkip = true;

// ---------------------------------------------------------------------------
// kernel 2: fused normal equations (lean form)
// ---------------------------------------------------------------------------
// The materialising kernel reproduces the reference's f32 operation order so that every output
// value can be compared with the reference bit for bit.  The fused pass has no per-point output to
// compare: its 45 sums per constraint are checked against the materialised sums to 1e-6.  It
// therefore keeps ONLY the discontinuous part of the reference's arithmetic exact -- the rigid
// transform and Interpolator::setIndexes/getQVector (locate_stage1: which cell a point falls in,
// and its fractional offsets, bit for bit) -- and evaluates everything that is a smooth function of
// (8 neighbours, offsets) in the cheapest association:
//   * the gradient as RCF:204-205's combination of the interp_table_ coefficients in nine FMAs (round 6; nested lerps over
//     the neighbours before: see eval_point_lean),
//   * the f64 detour of RCF:183-202 (doubles rounded into a float matrix) stays in f32,
//   * validity from the interpolated value itself: every neighbour enters it, so it is NaN exactly
//     when a neighbour is the NaN sentinel,
//   * -w/voxel_size folded into one scale, (dxs - dyc) and (dxc + dys) precomputed per constraint.
// Each of these differs from the reference's rounding by a few f32 ulp per point, with ONE exception that
// is kept in the reference's association: the interpolated value itself (interpolated_value, +32 VALU per
// point).  The residual d_ref - value amplifies a one-ulp difference in the value by |value / residual|,
// and where thousands of points share one local configuration (an axis-aligned plane: the same offsets and
// neighbours for every point) that difference has the same sign for all of them: with the value from the
// nested lerps the cost of such a constraint was off by up to 4.4e-5, J^T r by 2.2e-5
// (profiles/fuzz_reg_large.py, 1 440 constraints of 128^3 submaps; rows exact throughout).  Gradients have
// no such cancellation (they are differences of neighbours in both associations).  What must not happen in
// either kernel -- a point assigned to the neighbouring cell -- cannot, because locate_stage1 is shared.
// The 21 running products stay in f32 per thread across a tile (<= 2 * kReduceIters
// terms), widened to f64 for the wave / workgroup / constraint reduction: half the accumulator
// registers and no f64 FMA in the loop.  Fixed order throughout => bitwise reproducible.
__device__ __forceinline__ bool eval_point_lean(const float c[8], bool have, float Dx, float Dy, float Dz,
                                                float value, float inv_f, const PosePack& P, float xi, float yi,
                                                float d_ref, float w, float u[6]) {
#pragma clang fp contract(fast)
  // c = interp_table_ * distances^T, as interpolated_value made it (the reference's own coefficients, RCF:158): the
  // gradient is RCF:204-205's combination of them -- (c1 + c4 y + c6 z + c7 yz, c2 + c4 x + c5 z + c7 xz, c3 + c5 y +
  // c6 x + c7 xy) -- in nine FMAs.  Until round 6 the gradient came from a chain of nested lerps over the eight
  // neighbours (22 operations): its y and z components were differences of INTERPOLATED VALUES, i.e. carried an error of
  // an ulp of the distance (~1e-8 m) into a gradient of a few millimetres per voxel -- 2e-6 of it, which a constraint
  // with a dozen correspondences showed in its J^T r (profiles/fuzz_reg.py seed 300290: 1.27e-6 of the largest entry).
  // The coefficients are differences of neighbours throughout, as in the reference.
  const float q4 = Dx * Dy, q5 = Dy * Dz, q6 = Dz * Dx;
  const float gx = q5 * c[7] + (Dz * c[6] + (Dy * c[4] + c[1]));
  const float gy = q6 * c[7] + (Dz * c[5] + (Dx * c[4] + c[2]));
  const float gz = q4 * c[7] + (Dx * c[6] + (Dy * c[5] + c[3]));
  const float val = value;  // the reference's association (interpolated_value), computed by the caller
  const bool ok = have && (val == val);  // NaN sentinel among the neighbours <=> NaN value
  // What is accumulated is NOT u = (jo0, jo1, jo2, jo3, je3, r) itself but v = (h0, h1, h2, jo3, je3, r), h = -w / voxel_size *
  // gradient: (jo0, jo1) is (h0, h1) turned by the reading submap's yaw (RCF:214-218) -- a rotation the constraint's every point
  // shares, so reg_finalize_kernel applies it ONCE, in f64, to the sums of products (lean_basis: sum_u = T sum_v T^T with an
  // orthogonal T: nothing is amplified) instead of every point paying four operations for it.  jo3 and je3 are formed per point
  // as before: expressing them too through per-constraint constants (two point moments a = h0 x + h1 y, b = h1 x - h0 y) was
  // built and measured -- six more operations saved, -1 % -- and dropped: je3 = k . h - jo3 then comes out of the sums as a
  // difference of terms up to 25 x its size, and the large-constraint fuzzer's worst J^T J entry went from 2.9e-7 to 7.5e-7 of
  // the largest (profiles/r06_fused_gradient.txt).  Lanes without a correspondence carry zeros: the selects sit on the gradient.
  const float s = -w * inv_f;
  const float h0 = ok ? s * gx : 0.0f, h1 = ok ? s * gy : 0.0f, h2 = ok ? s * gz : 0.0f;
  const float mo3 = xi * P.sin_emo - yi * P.cos_emo;
  const float mo7 = xi * P.cos_emo + yi * P.sin_emo;
  u[0] = h0;
  u[1] = h1;
  u[2] = h2;
  u[3] = h0 * mo3 + h1 * mo7;
  u[4] = h0 * (P.k1 - mo3) + h1 * (P.k2 - mo7);
  u[5] = (d_ref - val) * w;
  return ok;
}

// u = T v (see eval_point_lean): row i of T, from the pose pack's own f32 values
__device__ __forceinline__ void lean_basis(const PosePack& P, double T[6][6]) {
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) T[i][j] = i == j ? 1.0 : 0.0;
  T[0][0] = (double)P.cos_e;  T[0][1] = -(double)P.sin_e;
  T[1][0] = (double)P.sin_e;  T[1][1] = (double)P.cos_e;
}

__device__ __forceinline__ void accumulate21(float acc[21], const float u[6]) {
#pragma clang fp contract(fast)
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b, ++k) acc[k] = u[a] * u[b] + acc[k];
}

// product 20 of accumulate21 (u[5] * u[5]) by itself: the cost-only pass's running sum
__device__ __forceinline__ void accumulate_square(float& acc, float r) {
#pragma clang fp contract(fast)
  acc = r * r + acc;
}

// Tiles are launched in an XCD-aware order (make_xcd_order); every tile still writes its partial
// sums into the slot it has in its constraint's own contiguous range (tile_first[c] + k-th tile of
// c), so the order in which a constraint's partials are summed never changes.
// COST_ONLY (vgx_reg_batch_evaluate_cost; registration_cost_function.cpp:179: the reference does no Jacobian work when
// `jacobians == nullptr`, and Ceres' Levenberg-Marquardt evaluates every trial step that way): the same walk over the
// same tiles with ONE running sum per lane -- the squared residual, the same f32 operations in the same order as product
// 20 of the full pass, reduced through the same tree -- so the cost it returns is the full pass's cost BIT FOR BIT, and a
// step accepted on the one is judged on the other's number.  No gradient, no pose-Jacobian products, a sixth of the
// accumulator registers, a one-sum epilogue.
template <int VPS, int LAYOUT, bool COST_ONLY>
__global__ __launch_bounds__(kBlockThreads, kLeanWaves) void reg_eval_reduce_lean_kernel(
    const ConstraintDev* __restrict__ cons, const PosePack* __restrict__ packs,
    const Tile* __restrict__ tiles, int n_tiles, const int32_t* __restrict__ tile_first,
    double* __restrict__ partials) {
  constexpr int PPT = kLeanPointsPerThread;
  constexpr int kIterPoints = kBlockThreads * PPT;
  static_assert(kChunkPoints % kIterPoints == 0, "an inner iteration never straddles a culling chunk");
  static_assert(kReduceIters * kTilePoints <= 64 * kChunkPoints, "one ballot covers a tile's chunks");
  const int t = blockIdx.x;
  if (t >= n_tiles) return;
  const Tile tile = tiles[t];
  const ConstraintDev& C = cons[tile.constraint];
  const PosePack P = packs[tile.constraint];
  const GridDev g = C.grid;
  const bool count_misses = C.no_corr_cost != 0.0;
  // sampling mode (RCF:113-122): residual i uses the point its weighted draw selects (made by
  // reg_draw_kernel before this launch: a batch always has sample_pts), with weight 1; draws are
  // scattered over the whole set, so there is nothing to cull
  const bool sampled = C.sample_raw != nullptr;
  const float4* bounds = (!count_misses && !sampled && C.chunk_bounds) ? C.chunk_bounds : nullptr;
  const long long chunk0 = tile.start / kChunkPoints;  // tiles start on chunk boundaries
  // Which of the tile's chunks can touch the reading grid: a 64-bit mask PER WAVEFRONT (one ballot), no LDS and no
  // barrier: the kernel needs no LDS of its own since round 6 (a tile's four wavefronts leave a row of sums each and the
  // finalize kernels add them).  What it is GIVEN at launch is another matter: launch_fused_tiles pads it with dynamic LDS
  // it never touches while the context integrates scans, to keep one workgroup's worth of registers free per CU.
  const int n_chunks = (tile.count + kChunkPoints - 1) / kChunkPoints;
  const int wlane = (int)(threadIdx.x & 63);
  const unsigned long long live =
      __ballot(wlane < n_chunks && !(bounds && chunk_outside(g, P, bounds[chunk0 + wlane])));
  auto chunk_live = [&](int k) { return ((live >> k) & 1ull) != 0ull; };
  constexpr int kAcc = COST_ONLY ? 1 : 21;
  float acc[kAcc];
#pragma unroll
  for (int k = 0; k < kAcc; ++k) acc[k] = 0.0f;
  const float nc = (float)C.no_corr_cost;
  const bool grid_empty = g.bricks == nullptr;

  f32x4 pt_next[PPT];
  float w_next[PPT];
  // the points of the iteration that starts at `base`: the sampling test stands round the loops, not inside them, so
  // that every point of an iteration is requested before the first is waited for (see load_tile_points)
  auto prefetch = [&](int base) {
    int64_t i[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int local = base + j * kBlockThreads + (int)threadIdx.x;
      i[j] = tile.start + (local < tile.count ? local : 0);
    }
    if (sampled) {
#pragma unroll
      for (int j = 0; j < PPT; ++j) pt_next[j] = as_global(reinterpret_cast<const f32x4*>(C.sample_pts))[C.row0 + i[j]];
#pragma unroll
      for (int j = 0; j < PPT; ++j) w_next[j] = 1.0f;  // RCF:121
    } else {
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        pt_next[j] = as_global(reinterpret_cast<const f32x4*>(C.xyzd))[i[j]];
        w_next[j] = as_global(C.weight)[i[j]];
      }
    }
  };
  bool live_next = chunk_live(0);
  if (live_next) prefetch(0);
  for (int base = 0; base < tile.count; base += kIterPoints) {
    f32x4 pt[PPT];
    float w[PPT];
    const bool live = live_next;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      pt[j] = pt_next[j];
      w[j] = w_next[j];
    }
    live_next = false;
    if (base + kIterPoints < tile.count) {
      live_next = chunk_live((base + kIterPoints) / kChunkPoints);
      if (live_next) prefetch(base + kIterPoints);
    }
    if (!live) continue;
    Located loc[PPT];
    bool have[PPT];
    float d[PPT][8];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      loc[j] = locate_stage1<VPS, LAYOUT>(g, P, pt[j].x, pt[j].y, pt[j].z);
      have[j] = false;
    }
    if (!grid_empty) {
      int slot[PPT];
#pragma unroll
      for (int j = 0; j < PPT; ++j) slot[j] = as_global(g.lut)[loc[j].lut_index];
      constexpr int CELLS = BrickLayout<VPS, LAYOUT>::cells;
      bool any = false;
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        have[j] = loc[j].inside && slot[j] >= 0;
        any |= have[j];
      }
      // a wavefront none of whose points found a reading block (the part of a live chunk that
      // sticks out of the reading grid) has nothing to gather or accumulate
      if (kBallotSkip && !count_misses && __builtin_amdgcn_ballot_w64(any) == 0ull) continue;
#pragma unroll
      for (int j = 0; j < PPT; ++j) {
        // 32-bit offsets: launch_brickify (vgx_context.hip) refuses a submap with n_blocks * CELLS >= 2^32
        const unsigned off = (unsigned)(have[j] ? slot[j] : 0) * (unsigned)CELLS + (unsigned)loc[j].cell_off;
        load_neighbours<VPS, LAYOUT>(g.bricks + off, d[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < PPT; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) d[j][k] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int local = base + j * kBlockThreads + (int)threadIdx.x;
      // branch-free: lanes without a correspondence carry zeros (or the miss cost) through the FMAs
      float u[6];
      const bool in_range = local < tile.count;
      float c_[8];
      const float value = interpolated_value(d[j], loc[j].Dx, loc[j].Dy, loc[j].Dz, c_[0], c_[1], c_[2], c_[3], c_[4],
                                             c_[5], c_[6], c_[7]);
      const bool ok = eval_point_lean(c_, have[j] && in_range, loc[j].Dx, loc[j].Dy, loc[j].Dz, value, g.voxel_size_inv, P,
                                      pt[j].x, pt[j].y, pt[j].w, w[j], u);
      // (u[0..4] are zeros without a correspondence: eval_point_lean)  RCF:165-166: w * no_correspondence_cost with zero
      // Jacobian rows
      u[5] = ok ? u[5] : ((count_misses && in_range) ? w[j] * nc : 0.0f);
      if (COST_ONLY) accumulate_square(acc[0], u[5]);   // (the five Jacobian entries are dead code here)
      else accumulate21(acc, u);
    }
  }
  // A tile leaves ONE ROW OF SUMS PER WAVEFRONT -- partials[tile slot][wave][22] -- and the finalize kernels add a tile's
  // four rows first, ((w0 + w1) + w2) + w3: the additions the workgroup made through LDS until round 5, in the same order
  // (bit for bit the same blocks), without LDS and without a barrier.
  const size_t row = ((size_t)tile_first[tile.constraint] + (size_t)(tile.start / C.tile_points)) * (kBlockThreads / 64) +
                     (threadIdx.x >> 6);
  if (COST_ONLY) {
    // the one sum over the 64 lanes (the pairing the reduce-scatter below uses for every sum: partners 32, 16, 8, 4, 2, 1
    // apart, a + b = b + a exactly) into entry 20 of the wavefront's row
    double v = (double)acc[0];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) partials[row * kPartialSize + 20] = v;
    return;
  }
  // The tile's 21 sums over its 64 lanes: a reduce-SCATTER butterfly.  Every step halves the sums a lane still carries --
  // it keeps one half, adds what its partner (lane ^ 32, 16, 8, 4, 2) sends of that half, and sends the other -- so 31
  // f64 exchanges instead of 21 x 6, and lane pair (2 s, 2 s + 1) ends up with sum s.  The additions are the ones the
  // plain butterfly makes for that sum, in the same pairing (a + b = b + a exactly): bit for bit the round-4 result.
  // The epilogue was most of what a tile costs beyond its points (round 4: 10 Ki-residual tiles +4 % on one GPU against
  // 20 Ki ones, the size a 1/8 shard wants -- VERDICT r4 item 6), and the f64 copies live together here only once the
  // point loop's registers are dead.
  const int lane = threadIdx.x & 63;
  {
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0, b2 = (lane & 4) != 0, b1 = (lane & 2) != 0;
    double r16[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {  // sums i (kept by lanes with bit 5 clear) and 16 + i (bit 5 set); 21 .. 31 do not exist
      const double lo = (double)acc[i], up = 16 + i < 21 ? (double)acc[16 + i < 21 ? 16 + i : 0] : 0.0;
      const double keep = b5 ? up : lo, send = b5 ? lo : up;
      r16[i] = keep + __shfl_xor(send, 32, 64);
    }
    double r8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double keep = b4 ? r16[8 + i] : r16[i], send = b4 ? r16[i] : r16[8 + i];
      r8[i] = keep + __shfl_xor(send, 16, 64);
    }
    double r4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double keep = b3 ? r8[4 + i] : r8[i], send = b3 ? r8[i] : r8[4 + i];
      r4[i] = keep + __shfl_xor(send, 8, 64);
    }
    double r2[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double keep = b2 ? r4[2 + i] : r4[i], send = b2 ? r4[i] : r4[2 + i];
      r2[i] = keep + __shfl_xor(send, 4, 64);
    }
    const double keep = b1 ? r2[1] : r2[0], send = b1 ? r2[0] : r2[1];
    double v = keep + __shfl_xor(send, 2, 64);
    v += __shfl_xor(v, 1, 64);
    const int s = lane >> 1;   // = 16 b5 + 8 b4 + 4 b3 + 2 b2 + b1
    if ((lane & 1) == 0 && s < 21) partials[row * kPartialSize + s] = v;
  }
}

// ---------------------------------------------------------------------------
// std::mt19937 streams on the device (sampling mode of the batched passes)
// ---------------------------------------------------------------------------
// One workgroup per engine: the 624-word state sits in LDS, each "twist" (the only sequential
// part of the generator) runs as three data-parallel phases -- mt[k] depends on the OLD mt[k],
// mt[k+1] and on mt[(k+397) % 624], which is old for k < 227 and already renewed afterwards, so
// [0,227), [227,454), [454,623) and the last word can each be computed in one step -- and the
// tempered outputs are written 256 at a time.  Bit for bit the stream Mt19937::operator() (and
// std::mt19937) produces; the state is left where the host engine can pick it up again.
struct StreamJobDev {
  uint32_t* state;  // Mt19937: 624 words + index
  uint32_t* out;
  long long count;
};

__device__ __forceinline__ uint32_t mt_twist_word(uint32_t cur, uint32_t next, uint32_t far) {
  const uint32_t y = (cur & 0x80000000u) | (next & 0x7fffffffu);
  return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// One workgroup per engine.  The twist  mt[k] = mt[(k + 397) mod 624] ^ f(mt[k], mt[k + 1])  splits
// into three ranges of 227 words in which word k of a later range needs the NEW word k - 227 of the
// range before it: thread t owns words t, 227 + t and 454 + t, so that chain stays in its registers.
// What it needs from other threads are OLD words only (k + 1 of each of its words, t + 397 for the
// first): four independent LDS reads of the previous block, one round trip.  New words go to a second
// LDS buffer (nobody's old value is overwritten), hence ONE barrier per twist -- it was three dependent
// LDS phases and seven barriers in place: 363 -> 216 us for the shipped configuration's 200 engines x
// 193 K outputs (a single-wave version without any s_barrier was slower, 709 us: too few lanes per phase).  Word 623 needs the new word 0: its owner recomputes that one itself.
constexpr int kMtThreads = 227;  // = H: one thread per word of a range, nobody idles behind an exec mask
// workgroup barrier that orders LDS accesses only (__syncthreads() also drains the global stores)
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__global__ __launch_bounds__(kMtThreads) void mt_generate_kernel(const StreamJobDev* __restrict__ jobs) {
  constexpr int N = Mt19937::kN, M = 397, H = N - M;  // H = 227
  constexpr int kLastOwner = N - 1 - 2 * H;            // thread 169 owns word 623 as its third
  constexpr int kStride = 3 * H + 3;                   // a block plus padding: threads 170 .. 226 "own" a third word too
  static_assert(kMtThreads == H, "one thread per word of a range");
  const StreamJobDev job = jobs[blockIdx.x];
  // The pointers come out of a struct in memory: generic as far as the compiler knows; told that they are
  // global, the stores go out as global_store_dword (a FLAT store also counts on lgkmcnt, which every
  // twist's barrier waits for).
  VGX_GLOBAL uint32_t* const g_out = (VGX_GLOBAL uint32_t*)job.out;
  VGX_GLOBAL uint32_t* const g_state = (VGX_GLOBAL uint32_t*)job.state;
  __shared__ uint32_t buf[2][kStride];
  const int t = threadIdx.x;
  for (int k = t; k < N; k += kMtThreads) buf[0][k] = g_state[k];
  for (int k = N + t; k < kStride; k += kMtThreads) buf[0][k] = buf[1][k] = 0u;
  int idx = (int)g_state[N];  // uniform; N = block used up
  int cur = 0;
  __syncthreads();
  const bool third = t <= kLastOwner;
  // this thread's words t, H + t, 2 H + t of the current block (2 H + t > 623: padding, never stored)
  uint32_t a = buf[0][t], b = buf[0][H + t], c = buf[0][2 * H + t];
  // One twist: this thread's three words of the next block from the current one (see above).  The loop a
  // single wavefront per SIMD issues instruction by instruction (nothing else runs on the CU), so it is kept
  // short and branch-free: every thread runs the third chain (threads beyond 169 on padding), and the one
  // special word -- 623 needs the NEW word 0 -- is a select: every thread recomputes word 0 from three
  // broadcast reads.
  auto twist = [&]() {
    const uint32_t* o = buf[cur];
    uint32_t* w = buf[cur ^ 1];
    const uint32_t a1 = o[t + 1], b1 = o[H + t + 1], far = o[t + M], c1 = o[2 * H + t + 1];
    const uint32_t new0 = mt_twist_word(o[0], o[1], o[M]);
    a = mt_twist_word(a, a1, far);
    b = mt_twist_word(b, b1, a);
    c = mt_twist_word(c, t == kLastOwner ? new0 : c1, b);  // (word 623: far = new word 396 = b, next = new word 0)
    w[t] = a;
    w[H + t] = b;
    w[2 * H + t] = c;
    lds_barrier();
    cur ^= 1;
  };
  // positions [idx, idx + take) of the current block go to out[produced ...] (a partial block: bounds checked)
  auto store_part = [&](long long produced, int take) {
    const int pa = t - idx, pb = H + t - idx, pc = 2 * H + t - idx;
    if (pa >= 0 && pa < take) g_out[produced + pa] = mt_temper(a);
    if (pb >= 0 && pb < take) g_out[produced + pb] = mt_temper(b);
    if (third && pc >= 0 && pc < take) g_out[produced + pc] = mt_temper(c);
  };
  long long produced = 0;
  // head: what is left of the block the engine stands in
  if (idx < N && produced < job.count) {
    const long long left = job.count - produced;
    const int take = (int)(left < (long long)(N - idx) ? left : (long long)(N - idx));
    store_part(produced, take);
    idx += take;
    produced += take;
  }
  // whole blocks: the loop a single wavefront per SIMD issues instruction by instruction (nothing else runs
  // on the CU), so it is kept short -- no bounds, one running pointer, the three stores at fixed offsets
  {
    VGX_GLOBAL uint32_t* p = g_out + produced + t;
    const long long blocks = (job.count - produced) / N;
    for (long long k = 0; k < blocks; ++k) {
      twist();
      p[0] = mt_temper(a);
      p[H] = mt_temper(b);
      if (third) p[2 * H] = mt_temper(c);
      p += N;
    }
    if (blocks > 0) idx = N;  // the last whole block is used up
    produced += blocks * N;
  }
  // tail: the first words of one more block
  if (produced < job.count) {
    twist();
    idx = 0;
    const int take = (int)(job.count - produced);
    store_part(produced, take);
    idx += take;
    produced += take;
  }
  __syncthreads();
  for (int k = t; k < N; k += kMtThreads) g_state[k] = buf[cur][k];
  if (t == 0) g_state[N] = (uint32_t)idx;
}

// Points a fused tile will really load at these poses (its chunks that survive the bounding-sphere
// test): the work estimate the XCD-aware launch order balances.  One wavefront per tile.
__global__ __launch_bounds__(64) void reg_tile_live_kernel(const ConstraintDev* __restrict__ cons,
                                                          const PosePack* __restrict__ packs,
                                                          const Tile* __restrict__ tiles, int n_tiles,
                                                          int32_t* __restrict__ live) {
  const int t = blockIdx.x;
  if (t >= n_tiles) return;
  const Tile tile = tiles[t];
  const ConstraintDev& C = cons[tile.constraint];
  const PosePack P = packs[tile.constraint];
  const bool cull = C.no_corr_cost == 0.0 && C.chunk_bounds && C.sample_raw == nullptr;
  const long long chunk0 = tile.start / kChunkPoints;
  const int n_chunks = (tile.count + kChunkPoints - 1) / kChunkPoints;
  int mine = 0;
  for (int k = threadIdx.x; k < n_chunks; k += 64) {
    const int pts = (k + 1) * kChunkPoints <= tile.count ? kChunkPoints : tile.count - k * kChunkPoints;
    if (!cull || !chunk_outside(C.grid, P, C.chunk_bounds[chunk0 + k])) mine += pts;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if (threadIdx.x == 0) live[t] = mine;
}

// Residuals the fused pass actually touches at these poses: the points of every chunk that
// survives the bounding-sphere test (the rest cost no memory traffic at all).  One thread per chunk.
__global__ void reg_count_live_kernel(const ConstraintDev* __restrict__ cons, const PosePack* __restrict__ packs,
                                      int n_cons, unsigned long long* __restrict__ live /* [n_cons] */) {
  const int c = blockIdx.x;
  if (c >= n_cons) return;
  const ConstraintDev& C = cons[c];
  const PosePack P = packs[c];
  const long long n_chunks = (C.n + kChunkPoints - 1) / kChunkPoints;
  unsigned long long mine = 0;
  const bool cull = C.no_corr_cost == 0.0 && C.chunk_bounds && C.sample_raw == nullptr;
  for (long long k = threadIdx.x; k < n_chunks; k += blockDim.x) {
    const long long pts = (k + 1) * kChunkPoints <= C.n ? kChunkPoints : C.n - k * kChunkPoints;
    if (!cull || !chunk_outside(C.grid, P, C.chunk_bounds[k])) mine += (unsigned long long)pts;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(live + c, mine);
}

// Groups of tiles -> one launch sequence in which every group sits on ONE XCD (workgroup p of a launch
// runs on XCD p % 8): heaviest group first onto the least loaded of 8 streams, so the XCDs finish
// together; launch position 8 i + x takes the i-th tile of stream x; a stream that has run dry lends
// its positions to the fullest one.
static std::vector<Tile> deal_to_xcds(const std::vector<std::vector<Tile>>& group_tiles,
                                      const std::vector<int64_t>& group_work, size_t n_tiles) {
  constexpr int kXcds = 8;
  std::vector<size_t> order(group_tiles.size());
  for (size_t g = 0; g < order.size(); ++g) order[g] = g;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return group_work[a] > group_work[b]; });
  std::vector<std::vector<Tile>> stream(kXcds);
  std::vector<int64_t> load(kXcds, 0);
  for (size_t g : order) {
    int best = 0;
    for (int x = 1; x < kXcds; ++x)
      if (load[(size_t)x] < load[(size_t)best]) best = x;
    stream[(size_t)best].insert(stream[(size_t)best].end(), group_tiles[g].begin(), group_tiles[g].end());
    load[(size_t)best] += group_work[g];
  }
  std::vector<size_t> next(kXcds, 0);
  std::vector<Tile> out;
  out.reserve(n_tiles);
  while (out.size() < n_tiles)
    for (int x = 0; x < kXcds && out.size() < n_tiles; ++x) {
      int src = x;
      if (next[(size_t)src] >= stream[(size_t)src].size()) {
        size_t left = 0;
        for (int y = 0; y < kXcds; ++y) {
          const size_t l = stream[(size_t)y].size() - next[(size_t)y];
          if (l > left) {
            left = l;
            src = y;
          }
        }
      }
      out.push_back(stream[(size_t)src][next[(size_t)src]++]);
    }
  return out;
}

// Launch order of the draw kernel: the sampling constraints of one reference point set search the same
// cumulative-weight array and bucket table (8 + ~12 B per point, a few MB per set).  All their tiles go
// to ONE XCD, back to back, so the tables are fetched into that XCD's L2 once and serve every draw of
// the set (shipped configuration: ~12 constraints x 8 K draws per set) instead of one HBM line per
// probe.  Draws are written by row: the order changes nothing but the time.
static std::vector<Tile> make_draw_order(const std::vector<ConstraintDev>& desc,
                                         const std::vector<int32_t>& tile_first, const std::vector<Tile>& tiles) {
  std::vector<const void*> key;
  std::vector<std::vector<Tile>> group_tiles;
  std::vector<int64_t> group_work;
  size_t n = 0;
  for (size_t c = 0; c < desc.size(); ++c) {
    if (!desc[c].sample_raw) continue;
    size_t g = 0;
    while (g < key.size() && key[g] != (const void*)desc[c].cumulative) ++g;
    if (g == key.size()) {
      key.push_back((const void*)desc[c].cumulative);
      group_tiles.emplace_back();
      group_work.push_back(0);
    }
    for (int32_t t = tile_first[c]; t < tile_first[c + 1]; ++t) {
      group_tiles[g].push_back(tiles[(size_t)t]);
      group_work[g] += tiles[(size_t)t].count;
      ++n;
    }
  }
  return deal_to_xcds(group_tiles, group_work, n);
}

// XCD-aware launch order of the fused pass's tiles.  Workgroup p of a launch runs on XCD p % 8
// (the dispatcher deals workgroups round the 8 XCDs), and every XCD has its own 4 MB L2.  The
// constraints that share a reference submap read the SAME point stream, chunk range by chunk range
// (config 3: ~6 per submap; the shipped mirrored configuration: ~12), so their tiles of one chunk
// range are placed on ONE XCD, next to each other in its dispatch sequence: they run at the same
// time and all but the first find the points in that XCD's L2 instead of going to the fabric.
// Groups (constraints with the same point array) are dealt to the 8 XCD streams heaviest first, by
// the points their tiles really load under chunk culling at the poses of the first evaluation (the
// pattern barely moves between solver iterations), so that the XCDs finish together; launch
// position 8 i + x takes the i-th tile of stream x.  Only the launch order changes: every tile
// writes its partial sums to its own slot, so results are bit for bit the same either way.
static bool make_xcd_order(const std::vector<ConstraintDev>& desc, const std::vector<int32_t>& tile_first,
                           const std::vector<int32_t>& tile_work, std::vector<Tile>& tiles, bool points_pass) {
  // VGX_POINTS_TILE_ORDER=0 keeps the materialising pass in plain constraint-major order.  Read per batch (not once per
  // process): bench.py measures one workload both ways in one process.
  if (points_pass) {
    const char* e = getenv("VGX_POINTS_TILE_ORDER");
    if (e && atoi(e) == 0) return false;
  }
  const int n = (int)desc.size();
  if (n < 2 || tiles.size() < 16) return false;
  // groups of constraints reading the same points (sampling constraints read scattered points: alone)
  std::vector<std::vector<int>> groups;
  {
    std::vector<std::pair<const void*, int>> key;  // (points, group)
    for (int c = 0; c < n; ++c) {
      int g = -1;
      if (!desc[(size_t)c].sample_raw)
        for (auto& k : key)
          if (k.first == (const void*)desc[(size_t)c].xyzd) g = k.second;
      if (g < 0) {
        g = (int)groups.size();
        groups.emplace_back();
        if (!desc[(size_t)c].sample_raw) key.emplace_back((const void*)desc[(size_t)c].xyzd, g);
      }
      groups[(size_t)g].push_back(c);
    }
  }
  // each group's tiles: chunk range major, constraint minor; its work = the points its tiles will
  // really load (chunk culling at the poses of the first evaluation) + a little per tile
  std::vector<std::vector<Tile>> group_tiles(groups.size());
  std::vector<int64_t> group_work(groups.size(), 0);
  for (size_t g = 0; g < groups.size(); ++g) {
    int most = 0;
    for (int c : groups[g]) most = std::max(most, tile_first[(size_t)c + 1] - tile_first[(size_t)c]);
    for (int r = 0; r < most; ++r)
      for (int c : groups[g])
        if (r < tile_first[(size_t)c + 1] - tile_first[(size_t)c]) {
          const size_t t = (size_t)tile_first[(size_t)c] + (size_t)r;
          group_tiles[g].push_back(tiles[t]);
          // bytes-ish: the materialising pass writes every row (36 B) and reads + gathers only where live
          group_work[g] += points_pass ? (int64_t)tiles[t].count * 36 + (int64_t)tile_work[t] * 52
                                       : (int64_t)tile_work[t] + 256;
        }
  }
  // How much of the point traffic is shareable at all: per (group, chunk range) everything beyond the
  // heaviest constraint's points could come out of the L2.  Measured: the
  // full-overlap workload (0.83 shareable) 4.03 -> 2.67 ms and 27.7 -> 11.9 GB of fabric reads; config 3
  // (constraints of a group overlap DIFFERENT parts of the reference, little to share) 1.66 -> 1.64 ms;
  // config 5 1.17 -> 1.42 ms: long runs of heavy and of culled tiles per XCD stall the in-order
  // dispatcher.  So the grouped order is used only where there is something to share (at least this
  // fraction of the loaded points) and little is culled (at least this fraction of all points loaded).
  constexpr double kOrderShareMin = 0.3;
  constexpr double kOrderLiveMin = 0.75;
  {
    int64_t total = 0, shareable = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
      int most = 0;
      for (int c : groups[g]) most = std::max(most, tile_first[(size_t)c + 1] - tile_first[(size_t)c]);
      for (int r = 0; r < most; ++r) {
        int64_t sum = 0, mx = 0;
        for (int c : groups[g])
          if (r < tile_first[(size_t)c + 1] - tile_first[(size_t)c]) {
            const int64_t w = tile_work[(size_t)tile_first[(size_t)c] + (size_t)r];
            sum += w;
            mx = std::max(mx, w);
          }
        total += sum;
        shareable += sum - mx;
      }
    }
    if (total == 0 || (double)shareable < kOrderShareMin * (double)total) return false;
    // ... and only when few tiles are culled: with long runs of culled (instant) and of heavy tiles in
    // one XCD's sequence the in-order dispatcher stalls the other XCDs (config 5 above: 56 % culled)
    int64_t all_points = 0;
    for (const Tile& t : tiles) all_points += t.count;
    if ((double)total < kOrderLiveMin * (double)all_points) return false;
  }
  std::vector<Tile> out = deal_to_xcds(group_tiles, group_work, tiles.size());
  tiles.swap(out);
  return true;
}

// One workgroup per constraint: 12 groups of 21 lanes sum the constraint's tile
// partials (group g takes tiles g, g+12, ... in order; the 12 group sums are added in
// group order: a fixed tree) and expand the 21 products into
// [cost, J^T r (8), upper J^T J (36)].
__global__ __launch_bounds__(256) void reg_finalize_kernel(const ConstraintDev* __restrict__ cons,
                                                          const PosePack* __restrict__ packs,
                                                          const int32_t* __restrict__ tile_first,
                                                          const double* __restrict__ partials,
                                                          double* __restrict__ normal) {
  const int c = blockIdx.x;
  constexpr int G = 12;
  __shared__ double part[G][21];
  __shared__ double s[21];
  const int grp = threadIdx.x / 21, k21 = threadIdx.x % 21;
  if (grp < G) {
    double v = 0.0;
    for (int t = tile_first[c] + grp; t < tile_first[c + 1]; t += G) {
      const double* w = partials + (size_t)t * (kBlockThreads / 64) * kPartialSize + k21;   // the tile's four wavefront rows
      v += ((w[0] + w[kPartialSize]) + w[2 * kPartialSize]) + w[3 * kPartialSize];
    }
    part[grp][k21] = v;
  }
  __syncthreads();
  if (threadIdx.x < 21) {
    double v = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) v += part[g][threadIdx.x];
    s[threadIdx.x] = v;
  }
  __syncthreads();
  // the sums are of products of v = (h0, h1, h2, jo3, je3, r): into products of u = T v (eval_point_lean, lean_basis), in f64,
  // every entry by the same fixed loop: sum_u(i, j) = sum_p sum_q T[i][p] T[j][q] sum_v(p, q).  Entry (5, 5) -- the cost --
  // is untouched (row 5 of T is e_5): the cost-only pass's number, bit for bit.
  __shared__ double su[21];
  if (threadIdx.x < 21) {
    double T[6][6];
    lean_basis(packs[c], T);
    int i = 0, rem = (int)threadIdx.x;
    while (rem >= 6 - i) {
      rem -= 6 - i;
      ++i;
    }
    const int j = i + rem;
    auto Sv = [&](int a, int b) {
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      return s[lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];
    };
    double acc = 0.0;
    if (i == 5 && j == 5) {
      acc = Sv(5, 5);
    } else {
      for (int p = 0; p < 6; ++p)
        for (int q = 0; q < 6; ++q) {
          const double t = T[i][p] * T[j][q];
          if (t != 0.0) acc += t * Sv(p, q);
        }
    }
    su[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 21) s[threadIdx.x] = su[threadIdx.x];
  __syncthreads();
  if (threadIdx.x < kNormalSize) {
    const int map[8] = {0, 1, 2, 3, 0, 1, 2, 4};
    const double sgn[8] = {1, 1, 1, 1, -1, -1, -1, 1};
    auto S = [&](int a, int b) {
      int i = a < b ? a : b, j = a < b ? b : a;
      return s[i * 6 - (i * (i - 1)) / 2 + (j - i)];
    };
    const double f = cons[c].factor;
    const double f2 = f * f;
    double v;
    int k = threadIdx.x;
    if (k == 0) {
      v = S(5, 5);
    } else if (k <= 8) {
      int p = k - 1;
      v = sgn[p] * S(map[p], 5);
    } else {
      int idx = k - 9, p = 0;
      while (idx >= 8 - p) {
        idx -= 8 - p;
        ++p;
      }
      int q = p + idx;
      v = sgn[p] * sgn[q] * S(map[p], map[q]);
    }
    normal[(size_t)c * kNormalSize + k] = v * f2;
  }
}

// The cost-only pass's finalize: slot 20 of the constraint's tile partials summed in reg_finalize_kernel's order (12
// strided groups, then the groups in order) and scaled by (N / sum w)^2 -- element 0 of the 45-block, bit for bit.
__global__ __launch_bounds__(64) void reg_finalize_cost_kernel(const ConstraintDev* __restrict__ cons, int n,
                                                              const int32_t* __restrict__ tile_first,
                                                              const double* __restrict__ partials, double* __restrict__ cost) {
  constexpr int G = 12;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 4), grp = threadIdx.x & 15;   // 16 lanes per constraint, 12 of them sum
  double v = 0.0;
  if (c < n && grp < G)
    for (int t = tile_first[c] + grp; t < tile_first[c + 1]; t += G) {
      const double* w = partials + (size_t)t * (kBlockThreads / 64) * kPartialSize + 20;
      v += ((w[0] + w[kPartialSize]) + w[2 * kPartialSize]) + w[3 * kPartialSize];
    }
  double total = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) total += __shfl(v, (int)(threadIdx.x & ~15u) + g, 64);
  if (c < n && grp == 0) {
    const double f = cons[c].factor;
    cost[c] = total * (f * f);
  }
}

// Deterministic scatter of per-constraint normal blocks into the all-reduce
// buffer: one thread per output element, looping over incident constraints.
__global__ void reg_assemble_kernel(const double* __restrict__ normal, int n, int csr_nodes,
                                    int n_nodes,
                                    const int32_t* __restrict__ node_pair,
                                    const int32_t* __restrict__ global_index,
                                    const int32_t* __restrict__ node_first,
                                    const int32_t* __restrict__ node_items,
                                    double* __restrict__ fused, int accumulate) {
  auto H = [&](const double* nb, int a, int b) {  // upper-triangular lookup
    int i = a < b ? a : b, j = a < b ? b : a;
    return nb[9 + i * 8 - (i * (i - 1)) / 2 + (j - i)];
  };
  const int64_t n_node_elems = (int64_t)csr_nodes * 20;  // 4 (J^T r) + 16 (diag block)
  const int64_t n_off = (int64_t)n * 16;
  if (blockIdx.x == gridDim.x - 1) {
    // the last workgroup only sums the costs: strided partial sums, then a fixed tree
    __shared__ double part[256];
    double v = 0.0;
    for (int c = threadIdx.x; c < n; c += 256) v += normal[(size_t)c * kNormalSize];
    part[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) fused[0] = accumulate ? fused[0] + part[0] : part[0];
    return;
  }
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid < n_node_elems) {
    int node = (int)(tid / 20), e = (int)(tid % 20);
    double v = 0.0;
    for (int it = node_first[node]; it < node_first[node + 1]; ++it) {
      int item = node_items[it];
      int c = item >> 1, side = item & 1;
      const double* nb = normal + (size_t)c * kNormalSize;
      if (e < 4) {
        v += nb[1 + 4 * side + e];
      } else {
        int k = (e - 4) / 4, l = (e - 4) % 4;
        v += H(nb, 4 * side + k, 4 * side + l);
      }
    }
    double* dst = e < 4 ? &fused[1 + 4 * (int64_t)node + e]
                        : &fused[1 + 4 * (int64_t)n_nodes + 16 * (int64_t)node + (e - 4)];
    *dst = accumulate ? *dst + v : v;
  } else if (tid < n_node_elems + n_off) {
    int64_t o = tid - n_node_elems;
    int c = (int)(o / 16), e = (int)(o % 16);
    const double* nb = normal + (size_t)c * kNormalSize;
    int gidx = global_index[c];
    double* dst = &fused[1 + 20 * (int64_t)n_nodes + 16 * (int64_t)gidx + e];
    double v = H(nb, e / 4, 4 + e % 4);
    *dst = accumulate ? *dst + v : v;
  }
}

// This shard's [n][45] blocks into rows global_index[c] of the [n_global][45] array every shard all-reduces:
// a row is written by exactly one shard and is zero everywhere else, so the SUM of the shards' arrays is
// exact whatever order a collective adds them in.
__global__ void reg_scatter_normal_kernel(const double* __restrict__ normal, int n, const int32_t* __restrict__ global_index,
                                          double* __restrict__ all) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (int64_t)n * kNormalSize) return;
  const int c = (int)(tid / kNormalSize), e = (int)(tid % kNormalSize);
  all[(size_t)global_index[c] * kNormalSize + e] = normal[tid];
}

// ---------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------
template <typename OUT>
static void launch_points(vgx_ctx ctx, int vps, int layout, const ConstraintDev* d_desc, const PosePack* d_pack,
                          const Tile* d_tiles, unsigned long long* d_tile_dead, int n_tiles, void* res, void* jr,
                          void* je, bool blocked, bool grouped) {
  if (n_tiles <= 0) return;
  // Aligned row stores (tile_local) put the point loads `shift` rows off their lines: a wavefront's 64 points and weights
  // touch 9 + 3 lines where they touched 8 + 2.  A launch that is bound by its row writes gains (config 3: -2.5 %, the
  // full-overlap workload in plain order -3.9 %); a launch in the grouped order, chosen where the constraints of a reference
  // submap find its points in one XCD's L2 and which is bound by those requests, loses (+12 %), so it keeps its loads
  // aligned (profiles/points_row_alignment.txt)
  const int shift_mask = grouped ? 0 : 63;
  hipLaunchKernelGGL(reg_points_tile_dead_kernel<kPointsPerThread>, dim3((n_tiles + 255) / 256), dim3(256), 0,
                     ctx->stream, d_desc, d_pack, d_tiles, n_tiles, d_tile_dead);
  dim3 grid(((n_tiles + 7) / 8) * 8), block(kBlockThreads);
  using O4 = typename Out4<OUT>::type;
  dispatch_brick(vps, layout, [&](auto V, auto L) {
    hipLaunchKernelGGL((reg_eval_points_kernel<V(), L(), OUT, kPointsPerThread>), grid, block, 0, ctx->stream, d_desc, d_pack, d_tiles,
                       (const uint32_t*)d_tile_dead, n_tiles, (OUT*)res, (O4*)jr, (O4*)je, blocked ? 1 : 0, shift_mask);
  });
}

template <typename OUT>
static void launch_points_single(hipStream_t stream, int vps, const ConstraintDev& desc, const PosePack& pack,
                                 void* res, void* jr, void* je) {
  const int n_tiles = (int)((desc.n + kTilePoints - 1) / kTilePoints);
  if (n_tiles <= 0) return;
  dim3 grid(((n_tiles + 7) / 8) * 8), block(kBlockThreads);
  using O4 = typename Out4<OUT>::type;
  dispatch_brick(vps, desc.grid.layout, [&](auto V, auto L) {
    hipLaunchKernelGGL((reg_eval_points_single_kernel<V(), L(), OUT, kPointsPerThread>), grid, block, 0, stream, desc, pack, n_tiles,
                       (OUT*)res, (O4*)jr, (O4*)je);
  });
}

// the visuals of the same evaluation: same grid, descriptor and pose pack as launch_points_single; cloud may be null
// (no residual cloud), arrows / origins are null together (no gradients)
static void launch_visuals_single(hipStream_t stream, int vps, const ConstraintDev& desc, const PosePack& pack,
                                  const VisualsPose& mission, void* cloud, double* arrows, double* origins) {
  const int n_tiles = (int)((desc.n + kTilePoints - 1) / kTilePoints);
  if (n_tiles <= 0 || (!cloud && !arrows)) return;
  dim3 grid(n_tiles), block(kBlockThreads);
  dispatch_brick(vps, desc.grid.layout, [&](auto V, auto L) {
    if (arrows)
      hipLaunchKernelGGL((reg_visuals_single_kernel<V(), L(), kPointsPerThread, true>), grid, block, 0, stream, desc, pack, mission,
                         n_tiles, (f32x4*)cloud, arrows, origins);
    else
      hipLaunchKernelGGL((reg_visuals_single_kernel<V(), L(), kPointsPerThread, false>), grid, block, 0, stream, desc, pack, mission,
                         n_tiles, (f32x4*)cloud, arrows, origins);
  });
}

// T_mission__reading as RCF:80-88 builds it: the reading pose narrowed to f32, minkindr's exp
static VisualsPose make_visuals_pose(const double read_pose[4]) {
  const YawQuat q = yaw_exp((float)read_pose[3]);
  return {q.w, q.z, (float)read_pose[0], (float)read_pose[1], (float)read_pose[2]};
}

}  // namespace vgx

// The cost-function visuals of the last vgx_reg_evaluate_visuals on this handle; the buffers grow on demand
struct vgx_reg_visuals_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  int64_t n_residual_points = 0, n_jacobians = 0;
  double factor = 0;
  vgx::DeviceBuffer d_cloud;    // [cap] 32-byte PointXYZI records
  vgx::DeviceBuffer d_arrows;   // double [cap][2][3]
  vgx::DeviceBuffer d_origins;  // double [cap][3]
};

using namespace vgx;

// ---------------------------------------------------------------------------
// single constraint
// ---------------------------------------------------------------------------
vgx::ConstraintDev vgx_reg_s::describe() const {
  ConstraintDev c;
  std::memset(&c, 0, sizeof(c));
  c.grid = reading->grid_dev(cfg.use_esdf_distance ? 1 : 0);
  const PointSet& ps = reference->points[cfg.registration_point_type];
  c.xyzd = ps.d_xyzd;
  c.weight = ps.d_weight;
  if (cfg.sampling_ratio != -1.0f) {
    c.sample_raw = d_sample_raw.as<uint32_t>();  // callers that stage elsewhere overwrite this
    c.cumulative = ps.d_cumulative;
    c.search_lut = ps.d_search_lut;
    c.search_buckets = ps.search_buckets;
    c.inv_order = ps.d_inv_order;
    c.n_points = ps.n;
  }
  c.chunk_bounds = ps.d_chunk_bounds;
  c.n = num_residuals;
  c.row0 = 0;
  c.prow0 = 0;
  // RCF:274: num_residuals / summed_reference_weight; sampled points weigh 1
  if (cfg.sampling_ratio != -1.0f) {
    c.factor = 1.0;
  } else {
    c.factor = ps.sum_weight != 0 ? (double)num_residuals / ps.sum_weight : 0.0;
  }
  c.no_corr_cost = cfg.no_correspondence_cost;
  return c;
}

// The engine outputs of one Evaluate: num_residuals draws of WeightedSampler::getRandomItem
// (weighted_sampler_inl.h:18-28, RCF:113-122) consume two 32-bit outputs each.  The engine is the
// reference submap's point-set engine, as in the reference (every cost function built on a submap
// advances the same stream), unless the caller asked for a private, separately seeded one.  Only
// the cheap sequential part stays on the host (~2 ns per output); the draw itself -- canonical
// double, scaling, binary search over the cumulative weights -- runs in the kernel.
vgx::SamplerEngine& vgx_reg_s::engine() {
  return cfg.sampler_seed != 0u ? rng : reference->points[cfg.registration_point_type].rng;
}

bool vgx_reg_s::points_current() const {
  const PointSet& ps = reference->points[cfg.registration_point_type];
  return ps.present && ps.version == points_version;
}

int vgx_reg_s::draw_raw(uint32_t* out) {
  SamplerEngine& e = engine();
  int rc = engine_to_host(ctx, e);  // a batched pass may have advanced the stream on the device
  if (rc != VGX_OK) return rc;
  const int64_t m = 2 * num_residuals;
  for (int64_t k = 0; k < m; ++k) out[k] = e.host();
  return VGX_OK;
}

// node -> incident (constraint << 1 | side), constraints in list order: the order reg_assemble_kernel sums in
static void build_node_csr(int n, const int32_t* node_pair, int csr_nodes, std::vector<int32_t>& first,
                           std::vector<int32_t>& items) {
  first.assign((size_t)csr_nodes + 1, 0);
  items.assign(2 * (size_t)n, 0);
  for (int c = 0; c < n; ++c)
    for (int s = 0; s < 2; ++s) first[(size_t)node_pair[2 * c + s] + 1]++;
  for (int i = 0; i < csr_nodes; ++i) first[(size_t)i + 1] += first[(size_t)i];
  std::vector<int32_t> cur(first.begin(), first.end() - 1);
  for (int c = 0; c < n; ++c)
    for (int s = 0; s < 2; ++s) items[(size_t)cur[(size_t)node_pair[2 * c + s]]++] = (c << 1) | s;
}

extern "C" {

void vgx_reg_config_default(vgx_reg_config* cfg) {
  if (!cfg) return;
  cfg->registration_point_type = VGX_POINTS_ISOSURFACE;
  cfg->sampling_ratio = -1.0f;
  cfg->no_correspondence_cost = 0.0;
  cfg->use_esdf_distance = 1;
  cfg->sampler_seed = 0u;  // share the reference submap's sampler stream (weighted_sampler.h:36-39)
}

int vgx_reg_create(vgx_ctx ctx, vgx_submap reference, vgx_submap reading, const vgx_reg_config* cfg,
                   vgx_reg* out) {
  if (!ctx || !out) return VGX_ERR_INVALID;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!reference || !reading || !cfg)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_create: NULL submap or config");
  if (reference->ctx != ctx || reading->ctx != ctx)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_create: submaps belong to another context");
  if (cfg->registration_point_type != VGX_POINTS_ISOSURFACE &&
      cfg->registration_point_type != VGX_POINTS_VOXELS)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_create: bad registration_point_type");
  const PointSet& ps = reference->points[cfg->registration_point_type];
  if (!ps.present)
    return set_error(ctx, VGX_ERR_INVALID,
                     "vgx_reg_create: reference submap has no registration points of that type "
                     "(submap not finished)");
  const int which = cfg->use_esdf_distance ? 1 : 0;
  if (reading->n_blocks > 0 && !reading->grid[which].present)
    return set_error(ctx, VGX_ERR_INVALID,
                     which ? "vgx_reg_create: reading submap has no ESDF layer"
                           : "vgx_reg_create: reading submap has no TSDF layer");
  if (reference->vps != reading->vps)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_reg_create: submaps differ in voxels_per_side");
  vgx_reg r = new (std::nothrow) vgx_reg_s();
  if (!r) return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_create: out of host memory");
  r->ctx = ctx;
  r->reference = reference;
  r->reading = reading;
  r->cfg = *cfg;
  r->points_version = ps.version;
  // RCF:45-55
  if (cfg->sampling_ratio != -1.0f) {
    r->num_residuals = (int64_t)(int)(cfg->sampling_ratio * (float)ps.n);
    if (r->num_residuals < 0) r->num_residuals = 0;
  } else {
    r->num_residuals = ps.n;
  }
  if (cfg->sampler_seed != 0u) r->rng.host.seed(cfg->sampler_seed);
  if (cfg->sampling_ratio != -1.0f && (int64_t)ps.cumulative_weight.size() != ps.n) {
    // points extracted on the device: build WeightedSampler's cumulative weights
    // (weighted_sampler_inl.h:5-16) from the device copy, in extraction order
    PointSet& mps = reference->points[cfg->registration_point_type];
    std::vector<float> w((size_t)mps.n);
    if (mps.n > 0 && (hipStreamSynchronize(ctx->stream) != hipSuccess ||
                      hipMemcpy(w.data(), mps.d_weight, (size_t)mps.n * sizeof(float),
                                hipMemcpyDeviceToHost) != hipSuccess)) {
      delete r;
      return set_error(ctx, VGX_ERR_HIP, "vgx_reg_create: weight download failed");
    }
    mps.cumulative_weight.resize((size_t)mps.n);
    double acc = 0;
    for (int64_t i = 0; i < mps.n; ++i) {
      acc = (i == 0) ? (double)w[0] : acc + (double)w[(size_t)i];
      mps.cumulative_weight[(size_t)i] = acc;
    }
  }
  if (cfg->sampling_ratio != -1.0f && ps.n == 0) r->num_residuals = 0;
  if (cfg->sampling_ratio != -1.0f && ps.n > 0) {
    PointSet& mps = reference->points[cfg->registration_point_type];
    hipError_t e = hipSuccess;
    if (!mps.d_cumulative) {
      // + 3 entries of padding (+inf): the draw probes cum[first .. first + 3] with two 16-byte loads and uses
      // only the entries inside its range, so it never has to clamp the addresses
      std::vector<double> padded(mps.cumulative_weight);
      padded.insert(padded.end(), 3, INFINITY);
      e = mps.d_cumulative.alloc_n(padded.size());
      if (e == hipSuccess)
        e = hipMemcpy(mps.d_cumulative, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !mps.d_search_lut) {
      // lut[k] = upper_bound(cumulative, (k / K) * total), k = 0 .. K, in the draw's own f64 arithmetic;
      // K = the power of two >= n (>= 4096): k / K and u * K are exact.  Targets ascend: one merge pass.
      int64_t K = kMinSearchBuckets;
      while (K < mps.n && K < kMaxSearchBuckets) K <<= 1;
      std::vector<int32_t> lut((size_t)K + 1);
      const std::vector<double>& cum = mps.cumulative_weight;
      const double total = cum.back();
      size_t pos = 0;
      for (int64_t k = 0; k <= K; ++k) {
        const double target = ((double)k / (double)K) * total;
        while (pos < cum.size() && !(target < cum[pos])) ++pos;  // first element > target
        lut[(size_t)k] = (int32_t)pos;
      }
      e = mps.d_search_lut.alloc_n(lut.size());
      if (e == hipSuccess)
        e = hipMemcpy(mps.d_search_lut, lut.data(), lut.size() * sizeof(int32_t), hipMemcpyHostToDevice);
      mps.search_buckets = (int32_t)K;
    }
    if (e == hipSuccess && !mps.inv_order.empty() && !mps.d_inv_order) {
      e = mps.d_inv_order.alloc_n((size_t)mps.n);
      if (e == hipSuccess)
        e = hipMemcpy(mps.d_inv_order, mps.inv_order.data(), (size_t)mps.n * sizeof(int32_t),
                      hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
      delete r;
      return set_error(ctx, VGX_ERR_HIP, std::string("vgx_reg_create: sampler tables: ") + hipGetErrorString(e));
    }
  }
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    ++reference->users;
    ++reading->users;
  }
  *out = r;
  return VGX_OK;
}

int vgx_reg_destroy(vgx_reg r) {
  if (!r) return VGX_ERR_INVALID;
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    if (r->users > 0) {  // a batch still lists it: the last vgx_reg_batch_destroy comes back here
      r->destroy_requested = true;
      return VGX_OK;
    }
  }
  (void)hipSetDevice(r->ctx->device);
  (void)hipStreamSynchronize(r->ctx->stream);
  // the submaps this cost function kept alive (vgx_submap_destroy was called on them while it existed)
  vgx_submap orphan[2] = {nullptr, nullptr};
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    vgx_submap both[2] = {r->reference, r->reading};
    for (int k = 0; k < 2; ++k) {
      vgx_submap sm = both[k];
      if (--sm->users == 0 && sm->destroy_requested) orphan[k] = sm;
    }
    if (orphan[0] == orphan[1]) orphan[1] = nullptr;  // a submap registered against itself
  }
  delete r;
  for (int k = 0; k < 2; ++k)
    if (orphan[k]) (void)vgx_submap_destroy(orphan[k]);
  return VGX_OK;
}

int64_t vgx_reg_num_residuals(vgx_reg r) { return r ? r->num_residuals : -1; }

static int reg_status(vgx_reg r) {
  // RCF:273: summed_reference_weight == 0 -> return false
  const PointSet& ps = r->reference->points[r->cfg.registration_point_type];
  double sw = r->cfg.sampling_ratio != -1.0f ? (double)r->num_residuals : ps.sum_weight;
  return sw == 0 ? VGX_EVALUATE_FALSE : VGX_OK;
}

namespace {
// Borrows an evaluation slot (must be called with ctx->mu held through `lk`); returns its index.
int acquire_slot(vgx_ctx ctx, std::unique_lock<std::mutex>& lk) {
  for (;;) {
    for (int k = 0; k < Context::kEvalSlots; ++k)
      if (!ctx->eval_slot[k].busy) {
        ctx->eval_slot[k].busy = true;
        return k;
      }
    ctx->slot_free.wait(lk);
  }
}
struct SlotLease {  // gives the slot back on every exit path; declare it BEFORE the context
                    // lock so that it is destroyed after the lock has been released
  vgx_ctx ctx;
  int k;
  ~SlotLease() {
    if (k < 0) return;
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      ctx->eval_slot[k].busy = false;
    }
    ctx->slot_free.notify_one();
  }
};
}  // namespace

// vgx_reg_evaluate, and -- with a visuals handle K (its lock held by the caller) -- vgx_reg_evaluate_visuals: the same
// evaluation plus one more kernel on the slot's stream that reads the same descriptor (the same engine outputs in
// sampling mode) and the same pose pack; the one host synchronisation below covers both.
static int reg_evaluate_impl(const char* fn, vgx_reg r, const double ref_pose[4], const double read_pose[4],
                             double* residuals, double* jac_ref, double* jac_read, vgx_reg_visuals K, bool want_cloud,
                             bool want_gradients) {
  vgx_ctx ctx = r->ctx;
  std::lock_guard<std::mutex> own(r->mu);
  const int64_t n = r->num_residuals;
  SlotLease lease{ctx, -1};
  std::unique_lock<std::mutex> lk(ctx->mu);  // launch under the context lock ...
  if (!residuals) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": residuals == NULL");
  if (!r->points_current())
    return set_error(ctx, VGX_ERR_INVALID,
                     std::string(fn) + ": the reference submap's registration points were replaced after "
                     "this cost function was created");
  const bool do_cloud = K && want_cloud;
  const bool do_grad = K && want_gradients && (jac_ref || jac_read);  // RCF:179: only when Jacobians were asked for
  if (K) {  // from here on the handle holds this evaluation's visuals, or none
    K->n_residual_points = 0;
    K->n_jacobians = 0;
    K->factor = 0;
  }
  if (n == 0) return reg_status(r);
  const int k = acquire_slot(ctx, lk);
  lease.k = k;
  Context::EvalSlot& sl = ctx->eval_slot[k];
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  if (!sl.stream) {
    VGX_HIP(ctx, hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
    VGX_HIP(ctx, hipEventCreateWithFlags(&sl.order, hipEventDisableTiming));
    VGX_HIP(ctx, sl.h_out.alloc(Context::kSmallOutputBytes));
  }
  VGX_HIP(ctx, sl.d_out.reserve((size_t)n * 9 * sizeof(double)));
  const bool sampled = r->cfg.sampling_ratio != -1.0f;
  if (sampled) {
    VGX_HIP(ctx, sl.d_raw.reserve((size_t)n * 2 * sizeof(uint32_t)));
    VGX_HIP(ctx, sl.h_raw.reserve((size_t)n * 2 * sizeof(uint32_t)));
  }
  if (do_cloud) {
    const hipError_t e = K->d_cloud.reserve((size_t)n * 32, 4096 * 32, true);
    if (e != hipSuccess) return alloc_error(ctx, e, "cost-function visuals: allocating the residual cloud");
  }
  if (do_grad && (size_t)n * 48 > K->d_arrows.bytes) {
    const size_t cap = (size_t)std::max<int64_t>(n + n / 4, 4096);
    const hipError_t e = alloc_group({{&K->d_arrows, cap * 48}, {&K->d_origins, cap * 24}});
    if (e != hipSuccess) return alloc_error(ctx, e, "cost-function visuals: allocating the Jacobian markers");
  }
  PosePack pack;
  make_pose_pack(ref_pose, read_pose, &pack);
  double* d_res = sl.d_out.as<double>();
  double* d_jr = jac_ref ? d_res + n : nullptr;
  double* d_je = jac_read ? d_res + 5 * n : nullptr;
  // everything already enqueued on the context stream (uploads, extraction) happens before this
  VGX_HIP(ctx, hipEventRecord(sl.order, ctx->stream));
  VGX_HIP(ctx, hipStreamWaitEvent(sl.stream, sl.order, 0));
  ConstraintDev desc = r->describe();
  if (sampled) {
    // this Evaluate's engine outputs (drawn under the lock: the engine is shared)
    const int rc_draw = r->draw_raw(sl.h_raw.as<uint32_t>());
    if (rc_draw != VGX_OK) return rc_draw;
    VGX_HIP(ctx, hipMemcpyAsync(sl.d_raw.p, sl.h_raw.p, (size_t)n * 2 * sizeof(uint32_t), hipMemcpyHostToDevice,
                                sl.stream));
    desc.sample_raw = sl.d_raw.as<uint32_t>();
  }
  if (reg_status(r) == VGX_EVALUATE_FALSE) return VGX_EVALUATE_FALSE;
  launch_points_single<double>(sl.stream, r->reading->vps, desc, pack, d_res, d_jr, d_je);
  if (do_cloud || do_grad)
    launch_visuals_single(sl.stream, r->reading->vps, desc, pack, make_visuals_pose(read_pose),
                          do_cloud ? K->d_cloud.p : nullptr, do_grad ? K->d_arrows.as<double>() : nullptr,
                          do_grad ? K->d_origins.as<double>() : nullptr);
  VGX_HIP(ctx, hipGetLastError());
  lk.unlock();
  // ... and copy + wait outside it: other cost functions' evaluations proceed meanwhile.  Small
  // outputs (the shipped sampled configuration: a few thousand residuals) come back in one copy
  // into the slot's pinned buffer and are scattered by the host; large ones go straight into the
  // caller's (pageable) arrays, three copies that block their caller.
  hipError_t e = hipSuccess;
  const size_t out_bytes = (size_t)n * 9 * sizeof(double);
  if (out_bytes <= Context::kSmallOutputBytes && sl.h_out.p) {
    e = hipMemcpyAsync(sl.h_out.p, d_res, out_bytes, hipMemcpyDeviceToHost, sl.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(sl.stream);
    if (e == hipSuccess) {
      const double* h_out = sl.h_out.as<double>();
      std::memcpy(residuals, h_out, (size_t)n * sizeof(double));
      if (jac_ref) std::memcpy(jac_ref, h_out + n, (size_t)n * 4 * sizeof(double));
      if (jac_read) std::memcpy(jac_read, h_out + 5 * n, (size_t)n * 4 * sizeof(double));
    }
  } else {
    e = hipMemcpyAsync(residuals, d_res, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, sl.stream);
    if (e == hipSuccess && jac_ref)
      e = hipMemcpyAsync(jac_ref, d_res + n, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, sl.stream);
    if (e == hipSuccess && jac_read)
      e = hipMemcpyAsync(jac_read, d_res + 5 * n, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, sl.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(sl.stream);
  }
  if (e != hipSuccess) {
    lk.lock();
    return set_error(ctx, VGX_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
  }
  if (K) {
    K->n_residual_points = do_cloud ? n : 0;
    K->n_jacobians = do_grad ? n : 0;
    K->factor = desc.factor;
  }
  return VGX_OK;
}

int vgx_reg_evaluate(vgx_reg r, const double ref_pose[4], const double read_pose[4],
                     double* residuals, double* jac_ref, double* jac_read) {
  if (!r || !ref_pose || !read_pose) return VGX_ERR_INVALID;
  return reg_evaluate_impl("vgx_reg_evaluate", r, ref_pose, read_pose, residuals, jac_ref, jac_read, nullptr, false, false);
}

int vgx_reg_evaluate_visuals(vgx_reg r, const double ref_pose[4], const double read_pose[4], double* residuals,
                             double* jac_ref, double* jac_read, int32_t want_residual_cloud, int32_t want_gradients,
                             vgx_reg_visuals K) {
  if (!r || !ref_pose || !read_pose) return VGX_ERR_INVALID;
  if (!K) return set_error(r->ctx, VGX_ERR_INVALID, "vgx_reg_evaluate_visuals: NULL visuals");
  if (K->ctx != r->ctx) return set_error(r->ctx, VGX_ERR_INVALID, "vgx_reg_evaluate_visuals: visuals of another context");
  std::lock_guard<std::mutex> out_lk(K->mu);
  return reg_evaluate_impl("vgx_reg_evaluate_visuals", r, ref_pose, read_pose, residuals, jac_ref, jac_read, K,
                           want_residual_cloud != 0, want_gradients != 0);
}

int vgx_reg_visuals_create(vgx_ctx ctx, vgx_reg_visuals* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_visuals_create: NULL argument");
  vgx_reg_visuals K = new (std::nothrow) vgx_reg_visuals_s;
  if (!K) return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_visuals_create: out of host memory");
  K->ctx = ctx;
  *out = K;
  return VGX_OK;
}

int vgx_reg_visuals_destroy(vgx_reg_visuals K) {
  if (!K) return VGX_ERR_INVALID;
  (void)hipSetDevice(K->ctx->device);
  delete K;
  return VGX_OK;
}

int vgx_reg_visuals_stats(vgx_reg_visuals K, int64_t* n_residual_points, int64_t* n_jacobians) {
  if (!K) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(K->mu);
  if (n_residual_points) *n_residual_points = K->n_residual_points;
  if (n_jacobians) *n_jacobians = K->n_jacobians;
  return VGX_OK;
}

int vgx_reg_visuals_download(vgx_reg_visuals K, void* cloud_bytes, double* arrow_points, double* origin_points,
                             double* factor) {
  if (!K) return VGX_ERR_INVALID;
  vgx_ctx ctx = K->ctx;
  std::lock_guard<std::mutex> lk(K->mu);
  if (factor) *factor = K->factor;
  if (K->n_residual_points == 0 && K->n_jacobians == 0) return VGX_OK;
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  // (the evaluation that filled the handle waited for its stream: the arrays are complete)
  if (cloud_bytes && K->n_residual_points > 0)
    VGX_HIP(ctx, hipMemcpy(cloud_bytes, K->d_cloud.p, (size_t)K->n_residual_points * 32, hipMemcpyDeviceToHost));
  if (arrow_points && K->n_jacobians > 0)
    VGX_HIP(ctx, hipMemcpy(arrow_points, K->d_arrows.p, (size_t)K->n_jacobians * 48, hipMemcpyDeviceToHost));
  if (origin_points && K->n_jacobians > 0)
    VGX_HIP(ctx, hipMemcpy(origin_points, K->d_origins.p, (size_t)K->n_jacobians * 24, hipMemcpyDeviceToHost));
  return VGX_OK;
}

int vgx_reg_visuals_device_pointers(vgx_reg_visuals K, const void** cloud, const double** arrow_points,
                                    const double** origin_points) {
  if (!K) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(K->mu);
  if (cloud) *cloud = K->n_residual_points > 0 ? K->d_cloud.p : nullptr;
  if (arrow_points) *arrow_points = K->n_jacobians > 0 ? K->d_arrows.as<double>() : nullptr;
  if (origin_points) *origin_points = K->n_jacobians > 0 ? K->d_origins.as<double>() : nullptr;
  return VGX_OK;
}

int vgx_reg_evaluate_device_f32(vgx_reg r, const double ref_pose[4], const double read_pose[4],
                                void* d_residuals, void* d_jac_ref, void* d_jac_read) {
  if (!r || !ref_pose || !read_pose) return VGX_ERR_INVALID;
  vgx_ctx ctx = r->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!d_residuals) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_evaluate_device_f32: residuals == NULL");
  if (!r->points_current())
    return set_error(ctx, VGX_ERR_INVALID,
                     "vgx_reg_evaluate_device_f32: the reference submap's registration points were replaced "
                     "after this cost function was created");
  // this entry point does not wait for its kernel: in sampling mode the previous call's upload of
  // the engine outputs must have left the pinned staging buffer before it is refilled
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t n = r->num_residuals;
  if (r->cfg.sampling_ratio != -1.0f && n > 0) {
    VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    VGX_HIP(ctx, r->d_sample_raw.reserve((size_t)n * 2 * sizeof(uint32_t)));
    VGX_HIP(ctx, r->h_sample_raw.reserve((size_t)n * 2 * sizeof(uint32_t)));
    const int rc_draw = r->draw_raw(r->h_sample_raw.as<uint32_t>());
    if (rc_draw != VGX_OK) return rc_draw;
    VGX_HIP(ctx, hipMemcpyAsync(r->d_sample_raw.p, r->h_sample_raw.p, (size_t)n * 2 * sizeof(uint32_t),
                                hipMemcpyHostToDevice, ctx->stream));
  }
  if (reg_status(r) == VGX_EVALUATE_FALSE) return VGX_EVALUATE_FALSE;
  PosePack pack;
  make_pose_pack(ref_pose, read_pose, &pack);
  launch_points_single<float>(ctx->stream, r->reading->vps, r->describe(), pack, d_residuals, d_jac_ref,
                              d_jac_read);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

// ---------------------------------------------------------------------------
// batch
// ---------------------------------------------------------------------------
int vgx_reg_batch_create(vgx_ctx ctx, int32_t n, const vgx_reg* regs, const int32_t* node_pair,
                         const int32_t* global_index, int32_t n_global, vgx_reg_batch* out) {
  if (!ctx || !out) return VGX_ERR_INVALID;
  *out = nullptr;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n < 0 || (n > 0 && (!regs || !node_pair)))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_create: bad n / NULL arrays");
  // n_global is the caller's: a shard that owns none (or few) of the global list's constraints still
  // assembles -- and zeroes -- the full-size buffer.  Only "no index, no size" means n_global = n.
  if (!global_index && n_global < n) n_global = n;
  if (n_global < n) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_create: n_global < n");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int vps = 0, layout = 0;
  for (int c = 0; c < n; ++c) {
    if (!regs[c] || regs[c]->ctx != ctx)
      return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_create: NULL or foreign constraint");
    if (!regs[c]->points_current())
      return set_error(ctx, VGX_ERR_INVALID,
                       "vgx_reg_batch_create: a reference submap's registration points were replaced after "
                       "its cost function was created");
    if (node_pair[2 * c] < 0 || node_pair[2 * c + 1] < 0)
      return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_create: negative node index");
    if (global_index && (global_index[c] < 0 || global_index[c] >= n_global))
      return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_create: global_index out of range");
    if (vps == 0) vps = regs[c]->reading->vps;
    if (regs[c]->reading->vps != vps)
      return set_error(ctx, VGX_ERR_UNSUPPORTED, "vgx_reg_batch_create: mixed voxels_per_side");
    const int lay = regs[c]->reading->grid[regs[c]->cfg.use_esdf_distance ? 1 : 0].layout;
    if (c == 0) layout = lay;
    if (lay != layout)
      return set_error(ctx, VGX_ERR_UNSUPPORTED,
                       "vgx_reg_batch_create: submaps with different brick layouts (vgx_ctx_set_brick_layout was "
                       "changed between their creation)");
  }
  // A batch whose constraints ALL sample evaluates scattered points: every line a neighbourhood touches is a
  // fetch of its own, so it reads QUAD bricks (a neighbourhood in 32 contiguous bytes), made on demand from
  // the submaps' apron bricks and kept with them (vgx_ctx_set_sampling_bricks; results never depend on it).
  bool quad_on_demand = n > 0 && layout == VGX_BRICKS_APRON && ctx->sampling_bricks == VGX_SAMPLING_BRICKS_QUAD;
  for (int c = 0; c < n && quad_on_demand; ++c) quad_on_demand = regs[c]->sampling();
  if (quad_on_demand) {
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    // Results never depend on the layout, so running out of memory for the second copy (4.25 x the apron bricks, kept for
    // the submap's lifetime: ~340 MB per dense 256^3 submap) must not cost the batch: the copies made for THIS batch are
    // given back and it reads the apron bricks everything else reads.
    std::vector<std::pair<vgx_submap, int>> made;
    for (int c = 0; c < n && quad_on_demand; ++c) {
      const int which = regs[c]->cfg.use_esdf_distance ? 1 : 0;
      const bool had = regs[c]->reading->grid[which].d_quad != nullptr;
      const int rc_q = regs[c]->reading->ensure_quad_grid(which);
      if (rc_q == VGX_OK) {
        if (!had && regs[c]->reading->grid[which].d_quad) made.emplace_back(regs[c]->reading, which);
        continue;
      }
      if (rc_q != VGX_ERR_NOMEM) return rc_q;
      VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the copies' kernels are in flight)
      for (auto& m : made) m.first->grid[m.second].d_quad.release();
      static bool told = false;
      if (!told) {
        told = true;
        fprintf(stderr, "libvoxgraph_amd: no memory for the quad bricks of a sampling batch (%s); it reads the apron bricks "
                        "instead -- same results, slower scattered evaluations\n", vgx_last_error(ctx));
      }
      set_error(ctx, VGX_OK, "no error");
      quad_on_demand = false;
    }
    if (quad_on_demand) layout = VGX_BRICKS_QUAD;
  }
  vgx_reg_batch b = new (std::nothrow) vgx_reg_batch_s();
  if (!b) return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_batch_create: out of host memory");
  vgx_reg_batch ex = b;
  b->ctx = ctx;
  b->n = n;
  b->n_global = n_global;
  b->layout = layout;
  b->regs.assign(regs, regs + n);
  b->node_pair.assign(node_pair, node_pair + 2 * (size_t)n);
  b->global_index.resize((size_t)n);
  for (int c = 0; c < n; ++c) b->global_index[(size_t)c] = global_index ? global_index[c] : c;
  b->row_offset.assign((size_t)n + 1, 0);
  std::vector<ConstraintDev> desc((size_t)n);
  std::vector<int32_t> tile_first((size_t)n + 1, 0), points_tile_first((size_t)n + 1, 0);
  // Fused-pass tile size: a function of the constraint alone, so that its partial sums -- f32 running products inside a
  // tile -- and therefore its 45 numbers are bit for bit the same whichever batch or shard it is evaluated in.  10 Ki
  // residuals for large constraints since round 5 (20 Ki before: a 1/8 shard of config 3 was 2.4 rounds of tiles on
  // 256 CUs x 6 resident workgroups and its slowest CU decided -- profiles/r04_shard_balance.json: 0.61-0.71 of linear at
  // N = 8 predicted; the smaller tile cost 4 % on one GPU until the tile's epilogue became a reduce-scatter butterfly,
  // reg_eval_reduce_lean_kernel), a fifth of the constraint for smaller ones so that the launch still has many tiles per
  // CU (shipped configuration, 8 K draws per constraint: 1.60 -> 1.40 ms).  NOT a fixed number of tiles per constraint
  // that is a multiple of 8: tile t runs on XCD t % 8 and chunk culling is spatially structured, so with 16 tiles per
  // constraint the same XCDs got the live tiles of every constraint (config 3 1.58 -> 1.77 ms).
  auto reduce_iters_of = [](int64_t n_residuals) {
    return (int)std::min<int64_t>(kReduceIters, std::max<int64_t>(1, n_residuals / ((int64_t)kTilePoints * 5)));
  };
  int max_node = -1;
  for (int c = 0; c < n; ++c) {
    desc[(size_t)c] = regs[c]->describe();
    if (quad_on_demand) {
      const Grid& gq = regs[c]->reading->grid[regs[c]->cfg.use_esdf_distance ? 1 : 0];
      if (gq.d_bricks) {  // (a reading submap without blocks keeps its null grid)
        desc[(size_t)c].grid.bricks = gq.d_quad;
        desc[(size_t)c].grid.layout = VGX_BRICKS_QUAD;
      }
    }
    desc[(size_t)c].row0 = b->row_offset[(size_t)c];
    desc[(size_t)c].prow0 = (int64_t)b->tiles.size() * kTilePoints;  // (the tiles so far are whole ones or a constraint's last)
    b->row_offset[(size_t)c + 1] = b->row_offset[(size_t)c] + regs[c]->num_residuals;
    std::vector<Tile> t = make_tiles(c, regs[c]->num_residuals, kTilePoints);
    points_tile_first[(size_t)c] = (int32_t)b->tiles.size();
    b->tiles.insert(b->tiles.end(), t.begin(), t.end());
    tile_first[(size_t)c] = (int32_t)ex->reduce_tiles.size();
    desc[(size_t)c].tile_points = kTilePoints * reduce_iters_of(regs[c]->num_residuals);
    std::vector<Tile> rt = make_tiles(c, regs[c]->num_residuals, desc[(size_t)c].tile_points);
    ex->reduce_tiles.insert(ex->reduce_tiles.end(), rt.begin(), rt.end());
    max_node = std::max(max_node, std::max(node_pair[2 * c], node_pair[2 * c + 1]));
  }
  tile_first[(size_t)n] = (int32_t)ex->reduce_tiles.size();
  points_tile_first[(size_t)n] = (int32_t)b->tiles.size();
  ex->host_desc = desc;            // (sample_raw is filled in below) for the launch order, made at the first evaluation
  ex->host_tile_first = tile_first;
  // Sampling constraints: group by engine (order of first appearance).  One evaluation of the
  // batch is one Evaluate of every constraint in list order, so the constraints of an engine
  // consume consecutive ranges of its stream, 2 words per residual (RCF:113-122).
  {
    std::vector<int> job_of((size_t)n, -1);
    for (int c = 0; c < n; ++c) {
      if (!regs[c]->sampling() || regs[c]->num_residuals == 0) continue;
      SamplerEngine* e = &regs[c]->engine();
      int j = 0;
      while (j < (int)b->stream_jobs.size() && b->stream_jobs[(size_t)j].engine != e) ++j;
      if (j == (int)b->stream_jobs.size()) b->stream_jobs.push_back({e, 0, 0});
      job_of[(size_t)c] = j;
      b->stream_jobs[(size_t)j].count += 2 * regs[c]->num_residuals;
    }
    int64_t total = 0;
    for (auto& j : b->stream_jobs) {
      j.offset = total;
      total += j.count;
    }
    b->any_sampling = total > 0;
    if (b->any_sampling) {
      if (b->d_raw.alloc((size_t)total * sizeof(uint32_t)) != hipSuccess ||
          b->d_drawn.alloc((size_t)b->row_offset[(size_t)n] * sizeof(float4)) != hipSuccess ||
          b->d_drawn_idx.alloc((size_t)b->row_offset[(size_t)n] * sizeof(int32_t)) != hipSuccess) {
        vgx_reg_batch_destroy(b);
        return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_batch_create: sampler stream buffer allocation failed");
      }
      std::vector<int64_t> used(b->stream_jobs.size(), 0);
      for (int c = 0; c < n; ++c) {
        const int j = job_of[(size_t)c];
        if (j < 0) continue;
        desc[(size_t)c].sample_raw = b->d_raw.as<uint32_t>() + b->stream_jobs[(size_t)j].offset + used[(size_t)j];
        desc[(size_t)c].sample_pts = b->d_drawn.as<float4>();  // this evaluation's drawn points, by row (reg_draw_kernel)
        used[(size_t)j] += 2 * regs[c]->num_residuals;
      }
      std::vector<StreamJobDev> jd(b->stream_jobs.size());
      for (size_t j = 0; j < jd.size(); ++j) {
        SamplerEngine* e = b->stream_jobs[j].engine;
        if (!e->d_state && e->d_state.alloc(sizeof(Mt19937)) != hipSuccess) {
          vgx_reg_batch_destroy(b);
          return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_batch_create: sampler state allocation failed");
        }
        jd[j] = {e->d_state, b->d_raw.as<uint32_t>() + b->stream_jobs[j].offset, (long long)b->stream_jobs[j].count};
      }
      if (b->d_stream_jobs.alloc(jd.size() * sizeof(StreamJobDev)) != hipSuccess ||
          hipMemcpy(b->d_stream_jobs.p, jd.data(), jd.size() * sizeof(StreamJobDev), hipMemcpyHostToDevice) != hipSuccess) {
        vgx_reg_batch_destroy(b);
        return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_batch_create: sampler job table upload failed");
      }
    }
  }
  ex->host_desc = desc;
  ex->host_points_tile_first = points_tile_first;
  // CSR: node -> (constraint << 1 | side)
  ex->csr_nodes = max_node + 1;
  std::vector<int32_t> first, items;
  build_node_csr(n, node_pair, ex->csr_nodes, first, items);
  int rc = upload_new(ctx, b->d_desc, desc.data(), desc.size() * sizeof(ConstraintDev));
  if (rc == VGX_OK) rc = upload_new(ctx, b->d_tiles, b->tiles.data(), b->tiles.size() * sizeof(Tile));
  if (rc == VGX_OK && !b->tiles.empty() && b->d_tile_dead.alloc(tile_dead_bytes(b->tiles.size())) != hipSuccess) rc = VGX_ERR_NOMEM;
  if (rc == VGX_OK && b->any_sampling) {
    const std::vector<Tile> dt = make_draw_order(desc, points_tile_first, b->tiles);
    b->n_draw_tiles = (int32_t)dt.size();
    rc = upload_new(ctx, b->d_draw_tiles, dt.data(), dt.size() * sizeof(Tile));
  }
  if (rc == VGX_OK) rc = upload_new(ctx, ex->d_reduce_tiles, ex->reduce_tiles.data(), ex->reduce_tiles.size() * sizeof(Tile));
  if (rc == VGX_OK) rc = upload_new(ctx, b->d_tile_first, tile_first.data(), tile_first.size() * sizeof(int32_t));
  if (rc == VGX_OK) rc = upload_new(ctx, b->d_node_pair, b->node_pair.data(), b->node_pair.size() * sizeof(int32_t));
  if (rc == VGX_OK) rc = upload_new(ctx, b->d_global_index, b->global_index.data(), b->global_index.size() * sizeof(int32_t));
  if (rc == VGX_OK) rc = upload_new(ctx, ex->d_node_first, first.data(), first.size() * sizeof(int32_t));
  if (rc == VGX_OK) rc = upload_new(ctx, ex->d_node_items, items.data(), items.size() * sizeof(int32_t));
  if (rc == VGX_OK && n > 0) {
    // (allocated once, in this order: the headline kernel's speed depends on where its arrays land)
    if (b->d_pack.alloc((size_t)n * sizeof(PosePack)) != hipSuccess ||
        b->pack_stage.reserve((size_t)n * sizeof(PosePack)) != hipSuccess ||
        b->d_partials.alloc(std::max<size_t>(1, ex->reduce_tiles.size()) * (kBlockThreads / 64) * kPartialSize * sizeof(double)) != hipSuccess ||
        b->d_normal.alloc((size_t)n * kNormalSize * sizeof(double)) != hipSuccess ||
        b->h_normal.alloc((size_t)n * kNormalSize * sizeof(double)) != hipSuccess)
      rc = set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_batch_create: device allocation failed");
  }
  if (rc != VGX_OK) {
    vgx_reg_batch_destroy(b);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    for (vgx_reg r : b->regs) ++r->users;
    b->holds_regs = true;
  }
  *out = b;
  return VGX_OK;
}

int vgx_reg_batch_destroy(vgx_reg_batch b) {
  if (!b) return VGX_ERR_INVALID;
  {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    if (b->users > 0) {  // a pose graph still lists it: carried out when the last one lets go (vgx_pose_graph.hip)
      b->destroy_requested = true;
      return VGX_OK;
    }
  }
  (void)hipSetDevice(b->ctx->device);
  (void)hipStreamSynchronize(b->ctx->stream);
  std::vector<vgx_reg> orphans;  // cost functions destroyed by their owner while this batch listed them
  if (b->holds_regs) {
    std::lock_guard<std::mutex> lt(lifetime_mu());
    for (vgx_reg r : b->regs)
      if (--r->users == 0 && r->destroy_requested) orphans.push_back(r);
  }
  for (vgx_reg r : orphans) (void)vgx_reg_destroy(r);
  delete b;
  return VGX_OK;
}

int64_t vgx_reg_batch_num_residuals(vgx_reg_batch b) { return b ? b->row_offset.back() : -1; }

int vgx_reg_batch_row_offsets(vgx_reg_batch b, int64_t* row_offset) {
  if (!b || !row_offset) return VGX_ERR_INVALID;
  std::copy(b->row_offset.begin(), b->row_offset.end(), row_offset);
  return VGX_OK;
}

// Start of one batched evaluation: the registration points every constraint was built on must still
// be there, and in sampling mode this evaluation's engine outputs are generated on the device.
static int batch_points_current(vgx_reg_batch b) {
  for (vgx_reg r : b->regs)
    if (!r->points_current())
      return set_error(b->ctx, VGX_ERR_INVALID,
                       "vgx_reg_batch: a reference submap's registration points were replaced after the "
                       "batch was created");
  return VGX_OK;
}

static int batch_begin(vgx_reg_batch b) {
  vgx_ctx ctx = b->ctx;
  int rc0 = batch_points_current(b);
  if (rc0 != VGX_OK) return rc0;
  if (!b->any_sampling) return VGX_OK;
  for (auto& j : b->stream_jobs) {
    int rc = engine_to_device(ctx, *j.engine);
    if (rc != VGX_OK) return rc;
  }
  hipLaunchKernelGGL(mt_generate_kernel, dim3((unsigned)b->stream_jobs.size()), dim3(kMtThreads), 0, ctx->stream,
                     b->d_stream_jobs.as<StreamJobDev>());
  VGX_HIP(ctx, hipGetLastError());
  // persistent: 8 x kDrawWgsPerXcdDefault workgroups walk the tile sequence; more workgroups than tiles: one per tile
  const int per_xcd = 8 * kDrawWgsPerXcdDefault < b->n_draw_tiles ? kDrawWgsPerXcdDefault : (b->n_draw_tiles + 7) / 8;
  const dim3 grid((unsigned)(8 * per_xcd));
  hipLaunchKernelGGL(reg_draw_kernel, grid, dim3(256), 0, ctx->stream, b->d_desc.as<ConstraintDev>(),
                     b->d_draw_tiles.as<Tile>(), (int)b->n_draw_tiles, per_xcd, b->d_drawn_idx.as<int32_t>());
  VGX_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(reg_gather_points_kernel, grid, dim3(256), 0, ctx->stream, b->d_desc.as<ConstraintDev>(),
                     b->d_draw_tiles.as<Tile>(), (int)b->n_draw_tiles, per_xcd, b->d_drawn_idx.as<int32_t>(),
                     b->d_drawn.as<float4>());
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

static int batch_nodes_within(vgx_reg_batch b, int32_t n_nodes) {
  for (int32_t v : b->node_pair)
    if (v >= n_nodes) return set_error(b->ctx, VGX_ERR_INVALID, "vgx_reg_batch: node index >= n_nodes");
  return VGX_OK;
}

// pose packs for every constraint -> pinned staging (double-buffered) -> device.
// No stream synchronisation: the host only waits until the H2D copy that last used
// this staging half has finished, so it prepares evaluation k+1 while k still runs.
static int batch_upload_packs(vgx_reg_batch b, const double* poses, int32_t n_nodes, int32_t* status) {
  vgx_ctx ctx = b->ctx;
  if (b->n == 0) return VGX_OK;
  const int rc_nodes = batch_nodes_within(b, n_nodes);   // before a staging half is taken: a refused call leaves the handle as it was
  if (rc_nodes != VGX_OK) return rc_nodes;
  int turn = 0;
  hipError_t waited = hipSuccess;
  PosePack* stage = static_cast<PosePack*>(b->pack_stage.next(&turn, &waited));
  VGX_HIP(ctx, waited);
  for (int c = 0; c < b->n; ++c) {
    int i = b->node_pair[2 * (size_t)c], j = b->node_pair[2 * (size_t)c + 1];
    make_pose_pack(poses + 4 * (size_t)i, poses + 4 * (size_t)j, &stage[c]);
    if (status) status[c] = reg_status(b->regs[(size_t)c]);
  }
  VGX_HIP(ctx, hipMemcpyAsync(b->d_pack.as<PosePack>(), stage, (size_t)b->n * sizeof(PosePack),
                              hipMemcpyHostToDevice, ctx->stream));
  VGX_HIP(ctx, b->pack_stage.record(turn, ctx->stream));
  return VGX_OK;
}

// One-time per batch and pass: per-tile live points at the poses just uploaded -> XCD-aware launch
// order (make_xcd_order decides whether it pays).  Results do not depend on the order: fused tiles
// write their own partial-sum slots, materialising tiles their own rows.
static int apply_launch_order(vgx_reg_batch b, const std::vector<Tile>& tiles, Tile* d_tiles,
                              const std::vector<int32_t>& tile_first, bool points_pass) {
  vgx_ctx ctx = b->ctx;
  bool& grouped = points_pass ? b->points_order_grouped : b->launch_order_grouped;
  const int n_tiles = (int)tiles.size();
  DeviceBuffer s_live;
  VGX_HIP(ctx, s_live.alloc((size_t)n_tiles * sizeof(int32_t)));
  hipLaunchKernelGGL(reg_tile_live_kernel, dim3(n_tiles), dim3(64), 0, ctx->stream, b->d_desc.as<ConstraintDev>(), b->d_pack.as<PosePack>(),
                     d_tiles, n_tiles, s_live.as<int32_t>());
  VGX_HIP(ctx, hipGetLastError());
  std::vector<int32_t> work((size_t)n_tiles);
  VGX_HIP(ctx, hipMemcpyAsync(work.data(), s_live.p, work.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<Tile> ordered = tiles;
  grouped = make_xcd_order(b->host_desc, tile_first, work, ordered, points_pass);
  VGX_HIP(ctx, hipMemcpy(d_tiles, ordered.data(), ordered.size() * sizeof(Tile), hipMemcpyHostToDevice));
  return VGX_OK;
}

// The head of every batched evaluation (the caller holds ctx->mu and has set the device): the point sets are current
// and the sampling constraints have drawn (batch_begin), then the pose packs and statuses of this evaluation.
// Everything that can REFUSE the call comes before the draw: a refused call is no Evaluate
// (registration_cost_function.cpp:113-122 draws inside Evaluate) and leaves every engine where it was.
static int batch_evaluation_begin(vgx_reg_batch b, const double* poses, int32_t n_nodes, int32_t* status) {
  int rc = batch_points_current(b);
  if (rc != VGX_OK) return rc;
  rc = batch_nodes_within(b, n_nodes);
  if (rc != VGX_OK) return rc;
  rc = batch_begin(b);
  return rc != VGX_OK ? rc : batch_upload_packs(b, poses, n_nodes, status);
}

}  // extern "C"

// One materialising pass of the whole batch into the caller's rows (same conditions): OUT rows, `blocked`: res == jr == je,
// one array of tile blocks.
template <typename OUT>
static int batch_points_pass(vgx_reg_batch b, const double* poses, int32_t n_nodes, void* res, void* jr, void* je, bool blocked,
                             int32_t* status) {
  vgx_ctx ctx = b->ctx;
  int rc = batch_evaluation_begin(b, poses, n_nodes, status);
  if (rc != VGX_OK) return rc;
  if (b->n == 0) return VGX_OK;
  if (!b->points_order_made && !b->tiles.empty()) {
    rc = apply_launch_order(b, b->tiles, b->d_tiles.as<Tile>(), b->host_points_tile_first, /*points_pass=*/true);
    if (rc != VGX_OK) return rc;
    b->points_order_made = true;
  }
  launch_points<OUT>(ctx, b->regs[0]->reading->vps, b->layout, b->d_desc.as<ConstraintDev>(), b->d_pack.as<PosePack>(),
                     b->d_tiles.as<Tile>(), b->d_tile_dead.as<unsigned long long>(), (int)b->tiles.size(), res, jr, je, blocked,
                     b->points_order_grouped);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

extern "C" {

int vgx_reg_batch_evaluate_points(vgx_reg_batch b, const double* poses, int32_t n_nodes,
                                  void* d_residuals, void* d_jac_ref, void* d_jac_read,
                                  int32_t* status) {
  if (!b || !poses) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!d_residuals) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_evaluate_points: residuals == NULL");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  return batch_points_pass<float>(b, poses, n_nodes, d_residuals, d_jac_ref, d_jac_read, /*blocked=*/false, status);
}

// The materialising pass in Ceres' own types: f64 rows, every value the reference's f64 (include/voxgraph_amd.h).
int vgx_reg_batch_evaluate_points_f64(vgx_reg_batch b, const double* poses, int32_t n_nodes, void* d_residuals,
                                      void* d_jac_ref, void* d_jac_read, int32_t* status) {
  if (!b || !poses) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!d_residuals) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_evaluate_points_f64: residuals == NULL");
  if (((uintptr_t)d_jac_ref | (uintptr_t)d_jac_read) & 31u)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_evaluate_points_f64: Jacobian arrays must be 32-byte aligned (one row)");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  return batch_points_pass<double>(b, poses, n_nodes, d_residuals, d_jac_ref, d_jac_read, /*blocked=*/false, status);
}

// One evaluation of every constraint as f64 rows KEPT BY THE BATCH, and the slice of one constraint fetched to the host:
// SURVEY.md 8b's "vgx_reg_fetch(h, residuals, jac_ref, jac_read) for the cached per-constraint slice" (include/voxgraph_amd.h).
constexpr int64_t kRowsMirrorLimit = (int64_t)2 << 30;   // bytes of rows up to which a pinned host mirror is kept

int vgx_reg_batch_evaluate_rows_f64(vgx_reg_batch b, const double* poses, int32_t n_nodes, int32_t want_jac_ref,
                                    int32_t want_jac_read, int32_t* status) {
  if (!b || !poses) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  const int64_t R = b->row_offset.back();
  // ONE critical section from the pass to the mirror's copies: no other thread's evaluation of this batch comes between the
  // rows on the device, what rows_have says of them and what the mirror holds
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes[3] = {(size_t)std::max<int64_t>(R, 1) * 8, (size_t)std::max<int64_t>(R, 1) * 32, (size_t)std::max<int64_t>(R, 1) * 32};
  const bool want[3] = {true, want_jac_ref != 0, want_jac_read != 0};
  for (int a = 0; a < 3; ++a)
    if (want[a] && !b->d_rows[a].p && b->d_rows[a].alloc(bytes[a]) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_batch_evaluate_rows_f64: no device memory for the batch's own rows");
    }
  if (!b->h_rows.p && R > 0 && R * 72 <= kRowsMirrorLimit && b->h_rows.alloc((size_t)R * 72) != hipSuccess)
    (void)hipGetLastError();   // no pinned memory: fetches copy their slices from the device
  b->rows_mirrored = false;
  const int rc = batch_points_pass<double>(b, poses, n_nodes, b->d_rows[0].p, want[1] ? b->d_rows[1].p : nullptr,
                                           want[2] ? b->d_rows[2].p : nullptr, /*blocked=*/false, status);
  if (rc != VGX_OK) return rc;
  b->rows_have[0] = true;
  b->rows_have[1] = want[1];
  b->rows_have[2] = want[2];
  if (b->h_rows.p && R > 0) {   // the whole evaluation in (up to) three copies behind the kernel: every fetch is a host copy
    VGX_HIP(ctx, hipMemcpyAsync(b->h_rows.p, b->d_rows[0].p, (size_t)R * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (b->rows_have[1])
      VGX_HIP(ctx, hipMemcpyAsync(b->h_rows.as<char>() + (size_t)R * 8, b->d_rows[1].p, (size_t)R * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (b->rows_have[2])
      VGX_HIP(ctx, hipMemcpyAsync(b->h_rows.as<char>() + (size_t)R * 40, b->d_rows[2].p, (size_t)R * 32, hipMemcpyDeviceToHost, ctx->stream));
    b->rows_mirrored = true;
  }
  return VGX_OK;
}

int vgx_reg_batch_fetch_rows_f64(vgx_reg_batch b, int32_t c, double* residuals, double* jac_ref, double* jac_read) {
  if (!b || c < 0 || c >= b->n) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!b->rows_have[0]) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_fetch_rows_f64: no rows evaluation to fetch from");
  if ((jac_ref && !b->rows_have[1]) || (jac_read && !b->rows_have[2]))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_fetch_rows_f64: the last rows evaluation was asked for no such Jacobian block");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the pass (and the mirror's copies) behind it
  const int64_t R = b->row_offset.back(), r0 = b->row_offset[(size_t)c], n = b->row_offset[(size_t)c + 1] - r0;
  if (n <= 0) return VGX_OK;
  if (b->rows_mirrored) {
    if (residuals) std::memcpy(residuals, b->h_rows.as<char>() + (size_t)r0 * 8, (size_t)n * 8);
    if (jac_ref) std::memcpy(jac_ref, b->h_rows.as<char>() + (size_t)R * 8 + (size_t)r0 * 32, (size_t)n * 32);
    if (jac_read) std::memcpy(jac_read, b->h_rows.as<char>() + (size_t)R * 40 + (size_t)r0 * 32, (size_t)n * 32);
    return VGX_OK;
  }
  if (residuals) VGX_HIP(ctx, hipMemcpy(residuals, b->d_rows[0].as<double>() + r0, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (jac_ref) VGX_HIP(ctx, hipMemcpy(jac_ref, b->d_rows[1].as<double>() + 4 * r0, (size_t)n * 32, hipMemcpyDeviceToHost));
  if (jac_read) VGX_HIP(ctx, hipMemcpy(jac_read, b->d_rows[2].as<double>() + 4 * r0, (size_t)n * 32, hipMemcpyDeviceToHost));
  return VGX_OK;
}

// The materialising pass into ONE array of tile blocks (include/voxgraph_amd.h): the same kernel, its three output pointers
// re-based per tile.
int vgx_reg_batch_blocked_layout(vgx_reg_batch b, int64_t* bytes, int32_t* rows_per_block, int64_t* first_block) {
  if (!b) return VGX_ERR_INVALID;
  if (bytes) *bytes = (int64_t)b->tiles.size() * kTilePoints * 36;
  if (rows_per_block) *rows_per_block = kTilePoints;
  if (first_block) {
    int64_t blk = 0;
    for (int c = 0; c < b->n; ++c) {
      first_block[c] = blk;
      blk += (b->regs[(size_t)c]->num_residuals + kTilePoints - 1) / kTilePoints;
    }
    first_block[b->n] = blk;
  }
  return VGX_OK;
}

int vgx_reg_batch_evaluate_points_blocked(vgx_reg_batch b, const double* poses, int32_t n_nodes, void* d_blocks,
                                          int32_t* status) {
  if (!b || !poses) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!d_blocks) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_evaluate_points_blocked: blocks == NULL");
  if (((uintptr_t)d_blocks & 15u) != 0)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_evaluate_points_blocked: blocks must be 16-byte aligned");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  return batch_points_pass<float>(b, poses, n_nodes, d_blocks, d_blocks, d_blocks, /*blocked=*/true, status);
}

// Placement by measurement (include/voxgraph_amd.h): which of the caller's candidate arrays the materialising pass runs
// fastest on.  First whole sets (k-th candidate of each array), then array by array against the best combination so far.
int vgx_reg_batch_choose_outputs(vgx_reg_batch b, const double* poses, int32_t n_nodes, int32_t n_candidates,
                                 void* const* d_residuals, void* const* d_jac_ref, void* const* d_jac_read, int32_t launches,
                                 int32_t chosen[3], float* ms_chosen, float* ms_trials) {
  if (!b || !poses || !d_residuals || !chosen || n_candidates <= 0 || launches <= 0) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  // Every trial is launches + 1 evaluations of the batch, and an evaluation of a SAMPLING batch draws: it would leave every
  // reference point set's std::mt19937 dozens of evaluations further on, silently -- "one evaluation of the batch = one
  // Evaluate of every constraint in list order" would no longer describe what the caller's next evaluation returns.  The
  // placement of the row arrays does not depend on which points are drawn: choose with an all-points batch of the same sizes.
  if (b->any_sampling)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_choose_outputs: a sampling batch (its trial evaluations would advance the "
                                           "sampling engines); choose the arrays with an all-points batch of the same sizes");
  for (int k = 0; k < n_candidates; ++k)
    if (!d_residuals[k] || (d_jac_ref && !d_jac_ref[k]) || (d_jac_read && !d_jac_read[k]))
      return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_choose_outputs: a candidate is NULL");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
      if (e0) (void)hipEventDestroy(e0);
      return set_error(ctx, VGX_ERR_HIP, "vgx_reg_batch_choose_outputs: hipEventCreate failed");
    }
  }
  int n_trials = 0;
  auto trial = [&](int i, int j, int k, float* ms) -> int {
    void* jr = d_jac_ref ? d_jac_ref[j] : nullptr;
    void* je = d_jac_read ? d_jac_read[k] : nullptr;
    int rc = vgx_reg_batch_evaluate_points(b, poses, n_nodes, d_residuals[i], jr, je, nullptr);  // warm-up (and first-use set-up)
    if (rc != VGX_OK) return rc;
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      VGX_HIP(ctx, hipEventRecord(e0, ctx->stream));
    }
    for (int l = 0; l < launches && rc == VGX_OK; ++l)
      rc = vgx_reg_batch_evaluate_points(b, poses, n_nodes, d_residuals[i], jr, je, nullptr);
    if (rc != VGX_OK) return rc;
    {
      std::lock_guard<std::mutex> lk(ctx->mu);
      VGX_HIP(ctx, hipEventRecord(e1, ctx->stream));
    }
    VGX_HIP(ctx, hipEventSynchronize(e1));
    float t = 0.0f;
    VGX_HIP(ctx, hipEventElapsedTime(&t, e0, e1));
    *ms = t / (float)launches;
    if (ms_trials) ms_trials[n_trials] = *ms;
    ++n_trials;
    return VGX_OK;
  };
  int rc = VGX_OK;
  float best = 0.0f;
  int pick[3] = {0, 0, 0};
  for (int s_ = 0; s_ < n_candidates && rc == VGX_OK; ++s_) {  // whole sets
    float t = 0.0f;
    rc = trial(s_, s_, s_, &t);
    if (rc == VGX_OK && (s_ == 0 || t < best)) {
      best = t;
      pick[0] = pick[1] = pick[2] = s_;
    }
  }
  // array by array (the larger ones first); a change is kept when it gains more than the measurement's own scatter
  for (int which = 2; which >= 0 && rc == VGX_OK && n_candidates > 1; --which) {
    if ((which == 1 && !d_jac_ref) || (which == 2 && !d_jac_read)) continue;
    const int set_pick = pick[which];
    for (int c = 0; c < n_candidates && rc == VGX_OK; ++c) {
      if (c == set_pick) {  // (measured as part of its set, or since adopted)
        if (ms_trials) ms_trials[n_trials] = -1.0f;
        ++n_trials;
        continue;
      }
      int q[3] = {pick[0], pick[1], pick[2]};
      q[which] = c;
      float t = 0.0f;
      rc = trial(q[0], q[1], q[2], &t);
      if (rc == VGX_OK && t < 0.995f * best) {
        best = t;
        pick[which] = c;
      }
    }
  }
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  if (rc != VGX_OK) return rc;
  chosen[0] = pick[0];
  chosen[1] = pick[1];
  chosen[2] = pick[2];
  if (ms_chosen) *ms_chosen = best;
  return VGX_OK;
}

// Row arrays chosen for their placement, allocated and released by the library (include/voxgraph_amd.h): n_candidates
// allocations of each array, vgx_reg_batch_choose_outputs over them, the unchosen ones freed.
int vgx_reg_batch_alloc_outputs(vgx_reg_batch b, const double* poses, int32_t n_nodes, int32_t n_candidates, int32_t want_jac_ref,
                                int32_t want_jac_read, void** d_residuals, void** d_jac_ref, void** d_jac_read, float* ms_chosen) {
  if (!b || !poses || !d_residuals || n_candidates <= 0 || n_candidates > 16 || (want_jac_ref && !d_jac_ref) ||
      (want_jac_read && !d_jac_read))
    return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  *d_residuals = nullptr;
  if (d_jac_ref) *d_jac_ref = nullptr;
  if (d_jac_read) *d_jac_read = nullptr;
  const size_t rows = (size_t)std::max<int64_t>(b->row_offset.back(), 1);
  DeviceBuffer cand[3][16];
  void* cand_p[3][16] = {};  // what vgx_reg_batch_choose_outputs reads
  const size_t bytes[3] = {rows * 4, rows * 16, rows * 16};
  const bool want[3] = {true, want_jac_ref != 0, want_jac_read != 0};
  int have = 0, rc = VGX_OK;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    VGX_HIP(ctx, hipSetDevice(ctx->device));
    for (; have < n_candidates; ++have) {
      bool ok = true;
      for (int a = 0; a < 3 && ok; ++a)
        if (want[a]) ok = cand[a][have].alloc(bytes[a]) == hipSuccess;
      if (!ok) {  // out of memory: choose among the complete sets there are (at least one is needed)
        (void)hipGetLastError();
        for (int a = 0; a < 3; ++a) cand[a][have].release();
        break;
      }
      for (int a = 0; a < 3; ++a) cand_p[a][have] = cand[a][have].p;
    }
  }
  if (have == 0) return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_batch_alloc_outputs: no memory for one set of row arrays");
  int32_t chosen[3] = {0, 0, 0};
  // (a sampling batch cannot be timed without advancing its engines -- vgx_reg_batch_choose_outputs refuses it: the first
  // set is kept as it is; a batch without rows has nothing to time)
  if (have > 1 && !b->any_sampling && b->row_offset.back() > 0)
    rc = vgx_reg_batch_choose_outputs(b, poses, n_nodes, have, cand_p[0], want[1] ? cand_p[1] : nullptr, want[2] ? cand_p[2] : nullptr, 3,
                                      chosen, ms_chosen, nullptr);
  else if (ms_chosen)
    *ms_chosen = 0.0f;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (rc == VGX_OK) {  // the chosen ones are the caller's from here (vgx_reg_batch_free_outputs)
      *d_residuals = cand[0][chosen[0]].detach();
      if (want[1]) *d_jac_ref = cand[1][chosen[1]].detach();
      if (want[2]) *d_jac_read = cand[2][chosen[2]].detach();
    }
    for (int a = 0; a < 3; ++a)
      for (int k = 0; k < have; ++k) cand[a][k].release();
  }
  return rc;
}

int vgx_reg_batch_free_outputs(vgx_reg_batch b, void* d_residuals, void* d_jac_ref, void* d_jac_read) {
  if (!b) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  // (the one raw free outside the owner types: vgx_reg_batch_alloc_outputs detached these arrays for the caller)
  for (void* p : {d_residuals, d_jac_ref, d_jac_read})
    if (p) (void)hipFree(p);
  return VGX_OK;
}

}  // extern "C"

// The fused pass's tile kernel (every solver evaluation): all 21 sums per tile, or -- cost_only -- the squared residual
// alone.  The caller holds ctx->mu and has uploaded the pose packs.
template <bool COST_ONLY>
static int launch_fused_tiles(vgx_reg_batch b) {
  vgx_ctx ctx = b->ctx;
  const int n_tiles = (int)b->reduce_tiles.size();
  if (!b->launch_order_made && n_tiles > 0) {
    int rc = apply_launch_order(b, b->reduce_tiles, b->d_reduce_tiles.as<Tile>(), b->host_tile_first, /*points_pass=*/false);
    if (rc != VGX_OK) return rc;
    b->launch_order_made = true;
  }
  // ROOM FOR A SCAN.  At 77 VGPRs the tile kernel is resident six workgroups deep on every CU (6 x 80 of a SIMD's 512
  // registers), and a racing TSDF scan's wavefronts need 104: while a solver evaluation ran, a scan submitted from the mapping
  // thread got a few workgroups in and the rest waited for the launch to drain -- 0.7 ms median, 1.4 ms worst (this kernel's
  // duration) against 0.1 ms alone; stream priorities changed nothing, nor did taking this kernel's own LDS away; the
  // workgroup stamps show the scan's workgroups starting over the whole 1.3 ms (profiles/r06_scan_latency.txt).  So while
  // the context has a TSDF integrator -- someone is mapping while this optimises, voxgraph_mapper.cpp:218-238 -- the kernel
  // is launched with 27 KB of dynamic LDS it never touches: FIVE resident workgroups per CU (160 KB / 27), 112 registers
  // free on every SIMD, room for one scan workgroup on every CU at any time: scans at 0.14-0.32 ms median / 0.22-0.45 ms
  // worst under a running solve, solver evaluations + 3 % (1.49 -> 1.53 ms).  Four per CU: 0.18 / 0.20 ms at + 12 %: not
  // taken.  Without an integrator on the context: no padding.
  const unsigned occupancy_pad = ctx->tsdf_integrators.load() > 0 ? 27u * 1024u : 0u;
  if (n_tiles > 0) {
    dim3 grid(n_tiles), block(kBlockThreads);
    dispatch_brick(b->regs[0]->reading->vps, b->layout, [&](auto V, auto L) {
      hipLaunchKernelGGL((reg_eval_reduce_lean_kernel<V(), L(), COST_ONLY>), grid, block, occupancy_pad, ctx->stream,
                         b->d_desc.as<ConstraintDev>(), b->d_pack.as<PosePack>(), b->d_reduce_tiles.as<Tile>(), n_tiles,
                         b->d_tile_first.as<int32_t>(), b->d_partials.as<double>());
    });
    VGX_HIP(ctx, hipGetLastError());
  }
  return VGX_OK;
}

extern "C" {

int vgx_reg_batch_evaluate_normal(vgx_reg_batch b, const double* poses, int32_t n_nodes,
                                  void* d_normal, double* normal_host, int32_t* status) {
  if (!b || !poses) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = batch_evaluation_begin(b, poses, n_nodes, status);
  if (rc != VGX_OK) return rc;
  if (b->n == 0) return VGX_OK;
  double* out = d_normal ? (double*)d_normal : b->d_normal.as<double>();
  if (!d_normal) b->normal_holds_blocks = false;   // until every launch below is queued
  rc = launch_fused_tiles<false>(b);
  if (rc != VGX_OK) return rc;
  hipLaunchKernelGGL(reg_finalize_kernel, dim3(b->n), dim3(256), 0, ctx->stream, b->d_desc.as<ConstraintDev>(), b->d_pack.as<PosePack>(),
                     b->d_tile_first.as<int32_t>(), b->d_partials.as<double>(), out);
  VGX_HIP(ctx, hipGetLastError());
  if (!d_normal) b->normal_holds_blocks = true;
  if (normal_host) {
    // through the batch's own PINNED block: a copy into the caller's pageable memory is staged by the runtime behind a
    // process-wide lock, and a scan submitted from the mapping thread meanwhile waited for this evaluation to finish
    // (profiles/r06_scan_latency.txt: 0.7 ms median per scan under a running solve, 0.1 ms with this)
    const size_t bytes = (size_t)b->n * kNormalSize * sizeof(double);
    VGX_HIP(ctx, hipMemcpyAsync(b->h_normal.as<double>(), out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(normal_host, b->h_normal.as<double>(), bytes);
  }
  return VGX_OK;
}

// One evaluation of every constraint's COST alone (include/voxgraph_amd.h): what Ceres asks for at every trial step
// (`jacobians == nullptr`, registration_cost_function.cpp:179).  cost[c] = r^T r of constraint c, already scaled by
// (N / sum w)^2: element 0 of vgx_reg_batch_evaluate_normal's 45-block at the same poses, bit for bit.
int vgx_reg_batch_evaluate_cost(vgx_reg_batch b, const double* poses, int32_t n_nodes, void* d_cost, double* cost_host,
                                int32_t* status) {
  if (!b || !poses) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = batch_evaluation_begin(b, poses, n_nodes, status);
  if (rc != VGX_OK) return rc;
  if (b->n == 0) return VGX_OK;
  // (the internal [n][45] array's first n doubles when the caller passes no device array: the blocks an earlier
  // vgx_reg_batch_evaluate_normal(d_normal == NULL) left there are gone, as the header says, and the flag makes
  // vgx_reg_batch_assemble / _scatter_normal(NULL) refuse to read the mix until the blocks are evaluated again)
  double* out = d_cost ? (double*)d_cost : b->d_normal.as<double>();
  if (!d_cost) b->normal_holds_blocks = false;
  rc = launch_fused_tiles<true>(b);
  if (rc != VGX_OK) return rc;
  hipLaunchKernelGGL(reg_finalize_cost_kernel, dim3((unsigned)((b->n + 3) / 4)), dim3(64), 0, ctx->stream, b->d_desc.as<ConstraintDev>(), (int)b->n,
                     b->d_tile_first.as<int32_t>(), b->d_partials.as<double>(), out);
  VGX_HIP(ctx, hipGetLastError());
  if (cost_host) {
    VGX_HIP(ctx, hipMemcpyAsync(b->h_normal.as<double>(), out, (size_t)b->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(cost_host, b->h_normal.as<double>(), (size_t)b->n * sizeof(double));
  }
  return VGX_OK;
}

int vgx_reg_batch_launch_order(vgx_reg_batch b, int32_t pass, int32_t* grouped) {
  if (!b || !grouped || (pass != 0 && pass != 1)) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(b->ctx->mu);
  const bool made = pass ? b->points_order_made : b->launch_order_made;
  *grouped = !made ? -1 : (int32_t)(pass ? b->points_order_grouped : b->launch_order_grouped);
  return VGX_OK;
}

// per constraint: residuals in chunks that survive the bounding-sphere test at the uploaded poses.  The two entry points
// below begin with batch_points_current + batch_upload_packs, NOT batch_evaluation_begin: they read chunk bounds and pose
// packs only, and a count is no evaluation -- batch_begin would draw, and leave every sampling engine one evaluation
// further on than the caller's next evaluation expects.
static int count_live_each(vgx_reg_batch b, std::vector<unsigned long long>& each) {
  vgx_ctx ctx = b->ctx;
  each.assign((size_t)b->n, 0);
  DeviceBuffer counter;
  VGX_HIP(ctx, counter.alloc((size_t)b->n * sizeof(unsigned long long)));
  VGX_HIP(ctx, hipMemsetAsync(counter.p, 0, (size_t)b->n * sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(reg_count_live_kernel, dim3(b->n), dim3(256), 0, ctx->stream, b->d_desc.as<ConstraintDev>(), b->d_pack.as<PosePack>(), b->n,
                     counter.as<unsigned long long>());
  VGX_HIP(ctx, hipGetLastError());
  VGX_HIP(ctx, hipMemcpyAsync(each.data(), counter.p, each.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VGX_OK;
}

int vgx_reg_batch_count_live_each(vgx_reg_batch b, const double* poses, int32_t n_nodes, int64_t* live_each) {
  if (!b || !poses || (b->n > 0 && !live_each)) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = batch_points_current(b);  // the chunk bounds read below belong to the point sets (no RNG advance)
  if (rc == VGX_OK) rc = batch_upload_packs(b, poses, n_nodes, nullptr);
  if (rc != VGX_OK || b->n == 0) return rc;
  std::vector<unsigned long long> each;
  rc = count_live_each(b, each);
  if (rc != VGX_OK) return rc;
  for (int c = 0; c < b->n; ++c) live_each[c] = (int64_t)each[(size_t)c];
  return VGX_OK;
}

int vgx_reg_batch_count_live(vgx_reg_batch b, const double* poses, int32_t n_nodes, int64_t* live_residuals,
                             int64_t* unique_points) {
  if (!b || !poses || !live_residuals) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  *live_residuals = 0;
  if (unique_points) *unique_points = 0;
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  int rc = batch_points_current(b);
  if (rc == VGX_OK) rc = batch_upload_packs(b, poses, n_nodes, nullptr);
  if (rc != VGX_OK) return rc;
  if (b->n == 0) return VGX_OK;
  std::vector<unsigned long long> each;
  rc = count_live_each(b, each);
  if (rc != VGX_OK) return rc;
  unsigned long long v = 0;
  for (unsigned long long e : each) v += e;
  *live_residuals = (int64_t)v;
  if (!unique_points) return VGX_OK;
  // Distinct registration points behind those residuals: constraints that share a reference submap
  // load the same points, and a point counts once however many of them load it.  Host arithmetic
  // (the same sphere test on downloaded chunk bounds): a measurement aid, not a hot path.
  std::vector<std::pair<const float4*, std::vector<float4>>> bounds;  // per distinct point set
  std::vector<std::pair<const float4*, std::vector<unsigned char>>> loaded;
  int64_t unique = 0;
  for (int c = 0; c < b->n; ++c) {
    const ConstraintDev& C = b->host_desc[(size_t)c];
    const int64_t n_chunks = (C.n + kChunkPoints - 1) / kChunkPoints;
    if (C.sample_raw) {  // scattered draws: every draw is its own load
      unique += C.n;
      continue;
    }
    size_t k = 0;
    while (k < bounds.size() && bounds[k].first != C.xyzd) ++k;
    if (k == bounds.size()) {
      bounds.emplace_back(C.xyzd, std::vector<float4>((size_t)n_chunks));
      loaded.emplace_back(C.xyzd, std::vector<unsigned char>((size_t)n_chunks, 0));
      if (n_chunks > 0 && C.chunk_bounds)
        VGX_HIP(ctx, hipMemcpy(bounds[k].second.data(), C.chunk_bounds, (size_t)n_chunks * sizeof(float4), hipMemcpyDeviceToHost));
    }
    const bool cull = C.no_corr_cost == 0.0 && C.chunk_bounds;
    PosePack P;
    make_pose_pack(poses + 4 * (size_t)b->node_pair[2 * (size_t)c], poses + 4 * (size_t)b->node_pair[2 * (size_t)c + 1], &P);
    for (int64_t q = 0; q < n_chunks; ++q)
      if (!cull || !chunk_outside(C.grid, P, bounds[k].second[(size_t)q])) loaded[k].second[(size_t)q] = 1;
  }
  for (size_t k = 0; k < loaded.size(); ++k) {
    // the point count of the set: n of any constraint that reads it (all-points constraints: n == set size)
    int64_t n_pts = 0;
    for (int c = 0; c < b->n; ++c)
      if (b->host_desc[(size_t)c].xyzd == loaded[k].first && !b->host_desc[(size_t)c].sample_raw)
        n_pts = std::max<int64_t>(n_pts, b->host_desc[(size_t)c].n);
    const int64_t n_chunks = (int64_t)loaded[k].second.size();
    for (int64_t q = 0; q < n_chunks; ++q)
      if (loaded[k].second[(size_t)q]) unique += (q + 1) * kChunkPoints <= n_pts ? kChunkPoints : n_pts - q * kChunkPoints;
  }
  *unique_points = unique;
  return VGX_OK;
}

int64_t vgx_reg_fused_size(int32_t n_nodes, int32_t n_global) {
  if (n_nodes < 0 || n_global < 0) return -1;
  return 1 + 20 * (int64_t)n_nodes + 16 * (int64_t)n_global;
}

int vgx_reg_batch_assemble(vgx_reg_batch b, const void* d_normal, int32_t n_nodes, void* d_fused,
                           int32_t zero_first) {
  if (!b || !d_fused) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  vgx_reg_batch ex = b;
  if (n_nodes < ex->csr_nodes)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_assemble: n_nodes smaller than the largest node index");
  if (!d_normal && b->n > 0 && !b->normal_holds_blocks)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_assemble: d_normal == NULL, and the batch's internal array holds no blocks "
                                           "(no vgx_reg_batch_evaluate_normal(d_normal == NULL) yet, or a cost-only evaluation since)");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const double* nb = d_normal ? (const double*)d_normal : b->d_normal.as<double>();
  if (zero_first)
    VGX_HIP(ctx, hipMemsetAsync(d_fused, 0, (size_t)vgx_reg_fused_size(n_nodes, b->n_global) * sizeof(double), ctx->stream));
  // nodes beyond the batch's CSR have no incident constraints: cover only the
  // CSR range for node elements, all constraints for the off-diagonal blocks.
  int64_t work = (int64_t)ex->csr_nodes * 20 + (int64_t)b->n * 16;
  if (work == 0) work = 1;
  int threads = 256;
  int blocks = (int)((work + threads - 1) / threads) + 1;  // + the cost-summing workgroup
  // The kernel indexes node elements by the CSR's node count but lays the
  // buffer out with the caller's n_nodes.
  hipLaunchKernelGGL(reg_assemble_kernel, dim3(blocks), dim3(threads), 0, ctx->stream, nb, b->n,
                     ex->csr_nodes, n_nodes, b->d_node_pair.as<int32_t>(), b->d_global_index.as<int32_t>(),
                     ex->d_node_first.as<int32_t>(), ex->d_node_items.as<int32_t>(),
                     (double*)d_fused, zero_first ? 0 : 1);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

int32_t vgx_reg_batch_brick_layout(vgx_reg_batch b) { return b ? (int32_t)b->layout : -1; }

int vgx_reg_batch_scatter_normal(vgx_reg_batch b, const void* d_normal, void* d_normal_all, int32_t zero_first) {
  if (!b || !d_normal_all) return VGX_ERR_INVALID;
  vgx_ctx ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!d_normal && b->n > 0 && !b->normal_holds_blocks)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_batch_scatter_normal: d_normal == NULL, and the batch's internal array holds no blocks "
                                           "(no vgx_reg_batch_evaluate_normal(d_normal == NULL) yet, or a cost-only evaluation since)");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  if (zero_first)
    VGX_HIP(ctx, hipMemsetAsync(d_normal_all, 0, (size_t)b->n_global * kNormalSize * sizeof(double), ctx->stream));
  if (b->n == 0) return VGX_OK;
  const double* nb = d_normal ? (const double*)d_normal : b->d_normal.as<double>();
  const int64_t work = (int64_t)b->n * kNormalSize;
  hipLaunchKernelGGL(reg_scatter_normal_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, ctx->stream, nb, b->n,
                     b->d_global_index.as<int32_t>(), (double*)d_normal_all);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

}  // extern "C"

// The whole constraint list's node structure on one context: assembles the fused buffer from the COMPLETE
// [n][45] array in list order -- the order a single vgx_reg_batch over the same list sums in, so the result
// does not depend on how the list was sharded (include/voxgraph_amd.h).
struct vgx_reg_assembler_s {
  vgx_ctx ctx = nullptr;
  int32_t n = 0, csr_nodes = 0;
  DeviceBuffer d_node_pair, d_identity, d_node_first, d_node_items;  // int32
};

extern "C" {

int vgx_reg_assembler_destroy(vgx_reg_assembler a) {
  if (!a) return VGX_ERR_INVALID;
  (void)hipSetDevice(a->ctx->device);
  (void)hipStreamSynchronize(a->ctx->stream);
  delete a;
  return VGX_OK;
}

int vgx_reg_assembler_create(vgx_ctx ctx, int32_t n, const int32_t* node_pair, vgx_reg_assembler* out) {
  if (!ctx || !out || n < 0 || (n > 0 && !node_pair)) return VGX_ERR_INVALID;
  *out = nullptr;
  int max_node = -1;
  for (int c = 0; c < 2 * n; ++c) {
    if (node_pair[c] < 0) return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_assembler_create: negative node index");
    max_node = std::max(max_node, node_pair[c]);
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  vgx_reg_assembler a = new (std::nothrow) vgx_reg_assembler_s();
  if (!a) return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_assembler_create: out of host memory");
  a->ctx = ctx;
  a->n = n;
  a->csr_nodes = max_node + 1;
  std::vector<int32_t> first, items, identity((size_t)n);
  build_node_csr(n, node_pair, a->csr_nodes, first, items);
  std::iota(identity.begin(), identity.end(), 0);
  if (upload_new(ctx, a->d_node_pair, node_pair, 2 * (size_t)n * 4) != VGX_OK ||
      upload_new(ctx, a->d_identity, identity.data(), (size_t)n * 4) != VGX_OK ||
      upload_new(ctx, a->d_node_first, first.data(), first.size() * 4) != VGX_OK ||
      upload_new(ctx, a->d_node_items, items.data(), items.size() * 4) != VGX_OK) {
    (void)hipGetLastError();
    vgx_reg_assembler_destroy(a);
    return set_error(ctx, VGX_ERR_NOMEM, "vgx_reg_assembler_create: device allocation failed");
  }
  *out = a;
  return VGX_OK;
}

int vgx_reg_assembler_assemble(vgx_reg_assembler a, const void* d_normal_all, int32_t n_nodes, void* d_fused) {
  if (!a || !d_fused || (a->n > 0 && !d_normal_all)) return VGX_ERR_INVALID;
  vgx_ctx ctx = a->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n_nodes < a->csr_nodes)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_reg_assembler_assemble: n_nodes smaller than the largest node index");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  VGX_HIP(ctx, hipMemsetAsync(d_fused, 0, (size_t)vgx_reg_fused_size(n_nodes, a->n) * sizeof(double), ctx->stream));
  int64_t work = (int64_t)a->csr_nodes * 20 + (int64_t)a->n * 16;
  if (work == 0) work = 1;
  const int blocks = (int)((work + 255) / 256) + 1;  // + the cost-summing workgroup
  hipLaunchKernelGGL(reg_assemble_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const double*)d_normal_all, a->n,
                     a->csr_nodes, n_nodes, a->d_node_pair.as<int32_t>(), a->d_identity.as<int32_t>(), a->d_node_first.as<int32_t>(),
                     a->d_node_items.as<int32_t>(),
                     (double*)d_fused, 0);
  VGX_HIP(ctx, hipGetLastError());
  return VGX_OK;
}

}  // extern "C"
