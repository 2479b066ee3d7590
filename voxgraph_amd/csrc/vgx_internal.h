// Internal host/device structures of libvoxgraph_amd.so (gfx950 only).
#ifndef VGX_INTERNAL_H_
#define VGX_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <mutex>
#include <condition_variable>
#include <initializer_list>
#include <random>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "voxgraph_amd.h"

namespace vgx {

// ---------------------------------------------------------------------------
// Device-visible descriptors (plain structs, copied by value)
// ---------------------------------------------------------------------------

// A finished layer re-laid for sampling: one "apron brick" per voxblox block,
// (vps+1)^3 floats, x fastest.  Cell (i,j,k) of brick b holds voxel (i,j,k) of
// block b for i,j,k < vps and the first voxel plane of the +x/+y/+z neighbour
// blocks for index == vps, so the 8 trilinear neighbours of any base voxel of
// block b live in ONE brick.  Invalid voxels (unobserved / zero weight /
// missing neighbour block) are stored as NaN: validity travels with the value.
// Brick layouts.  A context chooses one for the submaps it will hold (vgx_ctx_set_brick_layout):
//   0  apron brick (default): (vps+1)^3 floats, x fastest.  A neighbourhood is four 8-byte x-pairs in four
//      rows (y, z), (y, z+1), (y+1, z), (y+1, z+1): 68 B, 1156 B apart -> four cache lines.  1.2 x memory.
//      Fastest for the all-points passes (HBM / VALU bound: fewest bytes).
//   1  quad brick: for every x in [0, vps], y, z in [0, vps) the float4 {d(x,y,z), d(x,y+1,z), d(x,y,z+1),
//      d(x,y+1,z+1)}, x fastest.  A neighbourhood is two consecutive float4: 32 contiguous bytes, one or
//      two cache lines.  4.25 x memory.  Fastest where evaluations are scattered (sampling mode: every
//      touched line is an HBM fetch): -14 % per evaluation of the shipped configuration, +18-25 % on the
//      all-points passes (profiles/README.md, round 3).
// A third layout, 4^3 sub-tiles with their own aprons (2 x memory), was measured in between the two and not kept
// (profiles/README.md, "Brick layouts", row 2).
template <int VPS, int LAYOUT>
struct BrickLayout {
  static_assert(LAYOUT == 0 || LAYOUT == 1, "apron (0) or quad (1) bricks");
  static constexpr int B = VPS + 1;
  static constexpr int cells = LAYOUT == 0 ? B * B * B : B * VPS * VPS * 4;
  // float offset of a base voxel's neighbourhood anchor inside its brick
  __host__ __device__ static int anchor(int vx, int vy, int vz) {
    if (LAYOUT == 0) return vx + B * (vy + B * vz);
    return 4 * (vx + B * (vy + VPS * vz));
  }
  // brick float index -> apron cell (cx, cy, cz in [0, VPS])
  __host__ __device__ static void decode(int i, int& cx, int& cy, int& cz) {
    if (LAYOUT == 0) {
      cx = i % B; cy = (i / B) % B; cz = i / (B * B);
      return;
    }
    const int comp = i & 3, e = i >> 2;
    cx = e % B; cy = (e / B) % VPS + (comp & 1); cz = e / (B * VPS) + (comp >> 1);
  }
};
// The one place that enumerates (vps, layout): the two runtime values become compile-time ones, handed to a generic
// lambda as std::integral_constants -- f(V, L) names BrickLayout<V(), L()> or a kernel<V(), L(), ...>.  vps is 16 or 8
// (a submap of any other is refused when it is created), layout VGX_BRICKS_APRON or VGX_BRICKS_QUAD (vgx_ctx_set_brick_layout).
template <class F>
inline auto dispatch_brick(int vps, int layout, F&& f) {
  using std::integral_constant;
  if (vps == 16) {
    if (layout == VGX_BRICKS_QUAD) return f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
    return f(integral_constant<int, 16>{}, integral_constant<int, 0>{});
  }
  if (layout == VGX_BRICKS_QUAD) return f(integral_constant<int, 8>{}, integral_constant<int, 1>{});
  return f(integral_constant<int, 8>{}, integral_constant<int, 0>{});
}
inline size_t brick_cells(int vps, int layout) {
  return dispatch_brick(vps, layout, [](auto V, auto L) { return (size_t)BrickLayout<V(), L()>::cells; });
}

struct GridDev {
  const float* bricks;   // [n_blocks][BrickLayout<vps, layout>::cells]
  const int32_t* lut;    // dense block lookup [dim.z][dim.y][dim.x] -> brick or -1
  int32_t lut_min[3];
  int32_t lut_dim[3];
  float voxel_size, voxel_size_inv, block_size, block_size_inv;
  int32_t layout;        // brick layout of `bricks` (0 apron, 1 quad)
};

// A raw voxel layer's dense block table as the layer readers take it (vgx_interp.h's interp_base / interp_slot /
// layer_interp read exactly these fields): the descriptors of the map queries, the views, scan registration and
// localisation, the projected map and the isosurface points derive from it.  Filled only by submap_table (below) and
// live_layer_table (vgx_tsdf_internal.h).  GridDev above is the sampling grid's own form (int32_t[3], bricks).
struct LayerTable {
  const int32_t* lut;  // dense [dim.z][dim.y][dim.x]: the block's slot, negative when absent
  int3 lut_min, lut_dim;
  float voxel_size, voxel_size_inv, block_size, block_size_inv;
};

// Per-evaluation pose data of one constraint, computed on the host in the
// reference's own f32 arithmetic (registration_cost_function.cpp:69-110).
struct alignas(16) PosePack {
  float qw, qz;            // T_reading__reference rotation (yaw-only: x = y = 0)
  float tx, ty, tz;        // ... translation
  float cos_e, sin_e;      // cos/sin(yaw_reading)                    (.cpp:91-92)
  float cos_emo, sin_emo;  // cos/sin(yaw_reading - yaw_reference)    (.cpp:94-96)
  float dxs, dxc;          // (xe-xo)*sin_e , (xe-xo)*cos_e           (.cpp:225-226)
  float dys, dyc;          // (ye-yo)*sin_e , (ye-yo)*cos_e
  float k1, k2;            // dxs - dyc , dxc + dys (lean fused kernel)
  float pad;
};
static_assert(sizeof(PosePack) == 64, "PosePack must stay one 64-byte line");

// Static description of one constraint for the kernels.
struct alignas(16) ConstraintDev {
  GridDev grid;             // reading submap's sampling grid
  const float4* xyzd;       // reference submap's points {x,y,z,distance}
  const float* weight;      // ... weights
  // sampling mode (else all null): per residual two raw std::mt19937 outputs; the kernel turns
  // them into the WeightedSampler draw itself (generate_canonical -> * total -> upper_bound on the
  // cumulative weights -> optional Morton permutation), bit for bit what the host code did
  const uint32_t* sample_raw;
  const double* cumulative;   // [n_points] WeightedSampler::cumulative_item_weights_
  const int32_t* search_lut;  // [search_buckets + 1] first index of every draw bucket, or null
  int32_t search_buckets;     // K: a power of two
  const float4* sample_pts;   // batch: this evaluation's DRAWN POINTS {x,y,z,d}, by row (row0 + i); null: draw in place
  const int32_t* inv_order;   // uploaded index -> device index, or null
  int64_t n_points;
  const float4* chunk_bounds; // bounding spheres of consecutive kChunkPoints-point chunks
  int64_t n;                // num_residuals
  int64_t row0;             // first output row (stacked outputs)
  int64_t prow0;            // ... with every constraint padded to whole tiles: the blocked output layout (batch only)
  int32_t tile_points;      // batch: residuals per fused-pass tile of this constraint (all but its last tile)
  double factor;            // N / sum(w)                              (.cpp:274)
  double no_corr_cost;      // config.no_correspondence_cost
};

// A unit of work: `count` consecutive residuals of one constraint.
struct Tile {
  int32_t constraint;
  int32_t count;
  int64_t start;  // residual index within the constraint
};

// The weighted draw's std::upper_bound starts from a bucket table: with u = k / K the bound of
// u * total is precomputed, and upper_bound is monotone in its target, so the answer for any u in
// bucket k lies in [lut[k], lut[k + 1]].  K = the power of two >= n: the range holds about one
// element and the search becomes table load + four parallel loads, same result.
constexpr int kMinSearchBuckets = 4096;
constexpr int kMaxSearchBuckets = 1 << 24;
constexpr int kChunkPoints = 512;   // culling granule of the fused pass (= 256 threads x 2)
constexpr int kNormalSize = 45;     // per-constraint fused output (doubles)
constexpr int kPartialSize = 22;    // 21 unique products + reserved

// ---------------------------------------------------------------------------
// Owners of device and pinned host memory
// ---------------------------------------------------------------------------
// The one owner of device memory on the host side: frees in its destructor, so scratch declared in a function
// is freed on every exit path (the VGX_HIP macro returns early) and a handle's arrays go with the handle.  It neither
// synchronises nor zeroes: whoever frees an array that a queued kernel may still read synchronises that stream first.
struct DeviceBuffer {
  void* p = nullptr;
  size_t bytes = 0;  // capacity
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept { swap(o); }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    swap(o);
    return *this;
  }
  ~DeviceBuffer() { release(); }
  void swap(DeviceBuffer& o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  // exactly `n` bytes; what was held is freed first, and after a failure the buffer is empty
  hipError_t alloc(size_t n) {
    release();
    const hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    else p = nullptr;
    return e;
  }
  // grow-only: nothing when the capacity suffices, else max(n [+ n / 4], min_bytes) fresh bytes (the contents are lost)
  hipError_t reserve(size_t n, size_t min_bytes = 0, bool slack = false) {
    if (n <= bytes) return hipSuccess;
    return alloc(std::max(slack ? n + n / 4 : n, min_bytes));
  }
  // hands the array to the caller (who frees it) and leaves the buffer empty
  void* detach() {
    void* q = p;
    p = nullptr;
    bytes = 0;
    return q;
  }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};
// A DeviceBuffer with its element type: it reads as the T* it replaces (a kernel argument, a descriptor field, a null test),
// so only where no conversion is looked for -- an arm of ?:, a deduced template argument -- does a reader write get().
template <class T>
struct DeviceArray : DeviceBuffer {
  T* get() const { return static_cast<T*>(p); }
  operator T*() const { return get(); }
  hipError_t alloc_n(size_t count) { return alloc(count * sizeof(T)); }
};
// Pinned host memory, the same shape: staging buffers and host mirrors go with their handle.
struct PinnedBuffer {
  void* p = nullptr;
  size_t bytes = 0;  // capacity
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  PinnedBuffer(PinnedBuffer&& o) noexcept { swap(o); }
  PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
    swap(o);
    return *this;
  }
  ~PinnedBuffer() { release(); }
  void swap(PinnedBuffer& o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
  // exactly `n` bytes; what was held is freed first, and after a failure the buffer is empty
  hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
    release();
    const hipError_t e = hipHostMalloc(&p, n, flags);
    if (e == hipSuccess) bytes = n;
    else p = nullptr;
    return e;
  }
  // grow-only: nothing when the capacity suffices (the contents are lost otherwise)
  hipError_t reserve(size_t n) { return n <= bytes ? hipSuccess : alloc(n); }
  template <typename T>
  T* as() const {
    return static_cast<T*>(p);
  }
};
// The double-buffered pinned upload: two pinned halves filled in turn, so that the caller's (pageable) data is consumed
// when the call returns while the host-to-device copy runs behind it.  An event per half says when the copies that read
// it have finished and it may be filled again.  Like the buffers it never synchronises a stream: whoever lets `reserve`
// reallocate while a queued copy may still read a half synchronises that stream first.
struct UploadStage {
  PinnedBuffer half[2];
  hipEvent_t copied[2] = {nullptr, nullptr};
  int turn = 0;
  UploadStage() = default;
  UploadStage(const UploadStage&) = delete;
  UploadStage& operator=(const UploadStage&) = delete;
  ~UploadStage() {
    for (hipEvent_t e : copied)
      if (e) (void)hipEventDestroy(e);
  }
  size_t bytes() const { return half[0].bytes; }  // capacity of each half
  // grow-only, both halves; after a failure both are empty
  hipError_t reserve(size_t n) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k)
      if (!copied[k]) e = hipEventCreateWithFlags(&copied[k], hipEventDisableTiming);
    if (e == hipSuccess && n > bytes()) {
      half[0].release();
      half[1].release();
      e = half[0].alloc(n);
      if (e == hipSuccess) e = half[1].alloc(n);
    }
    if (e != hipSuccess) {
      half[0].release();
      half[1].release();
    }
    return e;
  }
  // the half to fill next, once the copies that last read it have finished; null (and *err) when that wait failed
  void* next(int* k, hipError_t* err = nullptr) {
    *k = turn;
    turn ^= 1;
    const hipError_t e = hipEventSynchronize(copied[*k]);
    if (err) *err = e;
    return e == hipSuccess ? half[*k].p : nullptr;
  }
  // after the copies that read half k have been queued on `stream`
  hipError_t record(int k, hipStream_t stream) { return hipEventRecord(copied[k], stream); }
};
// Arrays that share one capacity grow together: all are freed before the first is allocated (the peak does not rise while
// a handle grows), and after a failure all are empty.
struct DeviceBufferSize {
  DeviceBuffer* buffer;
  size_t bytes;
};
inline hipError_t alloc_group(std::initializer_list<DeviceBufferSize> group) {
  for (const DeviceBufferSize& g : group) g.buffer->release();
  hipError_t e = hipSuccess;
  for (const DeviceBufferSize& g : group)
    if (e == hipSuccess) e = g.buffer->alloc(g.bytes);
  if (e != hipSuccess)
    for (const DeviceBufferSize& g : group) g.buffer->release();
  return e;
}

// rocPRIM's two calls -- the size of the temporary storage with a null pointer, then the work with identical arguments --
// from ONE lambda hipError_t(void* tmp, size_t& bytes) that holds the rocPRIM call.  run_with_temp may reallocate `tmp`:
// only where nothing queued still uses it; launches that share a workspace ask with temp_bytes and make room once.
template <class Call>
hipError_t temp_bytes(Call& call, size_t* bytes) {
  *bytes = 0;
  return call(nullptr, *bytes);
}
template <class Call>
hipError_t run_with_temp(DeviceBuffer& tmp, Call& call) {
  size_t bytes = 0;
  hipError_t e = temp_bytes(call, &bytes);
  if (e == hipSuccess) e = tmp.reserve(bytes, 8);  // (never null: to rocPRIM a null workspace is the size query)
  if (e == hipSuccess) e = call(tmp.p, bytes);
  return e;
}

// ---------------------------------------------------------------------------
// Host objects behind the opaque handles
// ---------------------------------------------------------------------------
struct Context {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  std::mutex mu;
  // The TSDF path (the ACTIVE submap: layers, integrators, scans) has its own stream and its own lock, so that a scan
  // neither queues behind a solver evaluation on `stream` nor waits for `mu` while another thread evaluates -- the
  // reference integrates on the ROS thread while optimizePoseGraph runs on a std::async thread (voxgraph_mapper.cpp:
  // 236-238), and what makes that safe is the same here: finished submaps are immutable (voxgraph_mapper.cpp:464-471).
  // The two sides meet in vgx_submap_from_tsdf_layer (finishSubmap: the TSDF side's stream is waited for by an event).
  // Lock order where both are taken: integrator -> tsdf_mu -> mu.
  hipStream_t tsdf_own_stream = nullptr;
  hipStream_t tsdf_stream = nullptr;
  bool stream_priorities = false;  // own streams: TSDF side at the device's highest priority, registration side at its lowest
  std::atomic<int> tsdf_integrators{0};  // TSDF integrators alive on this context: the fused pass leaves room for their scans
  hipEvent_t ev_tsdf_start = nullptr, ev_tsdf_stop = nullptr, ev_handover = nullptr;
  std::mutex tsdf_mu;
  std::mutex err_mu;       // guards last_error only (set_error is called with and without `mu`)
  std::string last_error;
  int cu_count = 256;
  int brick_layout = 0;  // of the submaps created from now on (vgx_ctx_set_brick_layout)
  int sampling_bricks = 1;  // VGX_SAMPLING_BRICKS_QUAD: all-sampling batches read quad bricks made on demand
  // Evaluation slots of the drop-in Evaluate path.  A call takes a free slot for its duration
  // (stream, ordering event, device staging for the f64 outputs, pinned + device staging for the
  // sampler's engine outputs -- all grown on demand and reused), so constructing a cost function
  // allocates nothing: voxgraph rebuilds every registration constraint before each solve
  // (pose_graph_interface.cpp:149-175).  Ceres uses 4 threads (pose_graph.cpp:96); with 8 slots a
  // caller practically never waits.
  struct EvalSlot {
    hipStream_t stream = nullptr;
    hipEvent_t order = nullptr;
    DeviceBuffer d_out;        // [n][9] doubles
    DeviceBuffer d_raw;        // [2 n] engine outputs, and their pinned staging
    PinnedBuffer h_raw;
    PinnedBuffer h_out;        // kSmallOutputBytes: small evaluations come back in ONE copy
    bool busy = false;
  };
  static constexpr int kEvalSlots = 8;
  static constexpr size_t kSmallOutputBytes = 1u << 20;
  EvalSlot eval_slot[kEvalSlots];
  std::condition_variable slot_free;
};

// std::mt19937 (the engine of WeightedSampler, weighted_sampler.h:36-39) with its state in the
// open: the standard fixes the algorithm completely (seed 5489 -> 10000th output 4123659995), so
// this IS std::mt19937's stream, and the state can travel between the host and the device.
struct Mt19937 {
  static constexpr int kN = 624;
  uint32_t mt[kN];
  uint32_t idx = kN;  // next unread word of mt; kN = twist first (std::mt19937 after seed())
  Mt19937() { seed(5489u); }
  void seed(uint32_t s) {
    mt[0] = s;
    for (int i = 1; i < kN; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    idx = kN;
  }
  void twist() {
    for (int k = 0; k < kN; ++k) {
      uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % kN] & 0x7fffffffu);
      mt[k] = mt[(k + 397) % kN] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    idx = 0;
  }
  uint32_t operator()() {
    if (idx >= (uint32_t)kN) twist();
    uint32_t y = mt[idx++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};
static_assert(sizeof(Mt19937) == 625 * 4, "Mt19937 is copied to the device as 625 words");

// A sampler engine that lives wherever it was advanced last: the drop-in Evaluate draws on the
// host (a few thousand outputs per call), the batched passes generate whole streams on the device
// (mt_generate_kernel).  Exactly one copy is current at any time.
struct SamplerEngine {
  Mt19937 host;
  DeviceArray<uint32_t> d_state;  // 625 words, allocated at first device use
  bool on_device = false;       // the device copy is the current one
};

struct PointSet {
  int64_t n = 0;
  uint64_t version = 0;  // bumped whenever the points are replaced (cost functions remember theirs)
  DeviceArray<float4> d_xyzd;
  DeviceArray<float> d_weight;
  DeviceArray<float4> d_chunk_bounds;  // per kChunkPoints points: bounding sphere {cx,cy,cz,r}
  float aabb_min[3] = {0, 0, 0}, aabb_max[3] = {0, 0, 0};  // of the point positions (n > 0)
  double sum_weight = 0;
  bool present = false;
  std::vector<int64_t> order;            // order[i] = uploaded index of point i (empty = identity)
  std::vector<int32_t> inv_order;        // uploaded index -> device index (for sampling)
  std::vector<double> cumulative_weight; // WeightedSampler::cumulative_item_weights_ (upload order)
  DeviceArray<double> d_cumulative;      // device copy, made when a sampling cost function is created
  int32_t search_buckets = 0;
  DeviceArray<int32_t> d_search_lut;     // bucket table of the draw (search_buckets + 1 entries), same moment
  DeviceArray<int32_t> d_inv_order;      // device copy of inv_order (Morton-sorted sets only)
  // WeightedSampler's mutable engine (weighted_sampler.h:36-39): ONE default-seeded std::mt19937 per
  // point set, shared by every cost function that samples this set (vgx_reg_config.sampler_seed == 0)
  SamplerEngine rng;
};

struct Grid {
  DeviceArray<float> d_bricks;
  bool present = false;
  int layout = 0;  // the context's brick layout when this grid was built
  // the same grid as quad bricks, made on demand from the apron bricks for a batch whose constraints all
  // SAMPLE (scattered evaluations: a neighbourhood in 32 contiguous bytes; vgx_ctx_set_sampling_bricks)
  DeviceArray<float> d_quad;
};

}  // namespace vgx

struct vgx_ctx_s : vgx::Context {};

struct vgx_submap_s {
  vgx_ctx ctx = nullptr;
  int32_t id = 0;
  float voxel_size = 0, voxel_size_inv = 0, block_size = 0, block_size_inv = 0;
  int32_t vps = 0;
  int32_t n_blocks = 0;
  std::vector<int32_t> block_index;  // host copy [n][3]
  vgx::DeviceArray<int32_t> d_block_index;
  vgx::DeviceArray<int32_t> d_lut;
  int32_t lut_min[3] = {0, 0, 0};
  int32_t lut_dim[3] = {0, 0, 0};
  // raw layers (voxblox layout), kept for point extraction
  vgx::DeviceArray<float> d_tsdf_distance;
  vgx::DeviceArray<float> d_tsdf_weight;
  // the TSDF voxels' colours, one packed word per voxel (bytes r g b a, r lowest: TsdfLayerDev::rgba), or null: only a
  // submap that asked for them pays the 4 B per voxel (vgx_submap_from_tsdf_layer_colored, vgx_submap_set_colors)
  vgx::DeviceArray<uint32_t> d_tsdf_rgba;
  vgx::DeviceArray<float> d_esdf_distance;
  vgx::DeviceArray<uint8_t> d_esdf_observed;
  vgx::Grid grid[2];       // [0] TSDF, [1] ESDF sampling grids
  vgx::PointSet points[2]; // by VGX_POINTS_*
  std::vector<int32_t> isosurface_blocks;  // block slots holding isosurface vertices (VSM:237-240)
  vgx::DeviceArray<int32_t> d_iso_block_index;  // [isosurface_blocks.size()][3]
  // per block: 1 if any voxel of the raw TSDF layer has weight > 0 (vgx_project.hip), computed at first use and kept:
  // a finished submap is immutable, and the flags stay valid after vgx_submap_release_raw_layers
  vgx::DeviceArray<uint8_t> d_block_has_data;
  vgx::GridDev grid_dev(int which) const;
  int ensure_quad_grid(int which);  // apron bricks -> quad bricks, once (vgx_context.hip)
  // Lifetime (guarded by vgx::lifetime_mu()): cost functions made from this submap.  vgx_submap_destroy while users > 0
  // only records the request; the last vgx_reg_destroy carries it out (the reference's cost function holds
  // VoxgraphSubmap::ConstPtr: registration_cost_function.h -- a submap outlives every cost function built on it).
  int users = 0;
  bool destroy_requested = false;
};

namespace vgx {
// a finished submap's block table.  A submap with no blocks gets lut_dim = 0: every lookup misses.
inline LayerTable submap_table(const vgx_submap_s* sm) {
  LayerTable t{};
  t.lut = sm->d_lut;
  t.lut_min = make_int3(sm->lut_min[0], sm->lut_min[1], sm->lut_min[2]);
  if (sm->n_blocks > 0) t.lut_dim = make_int3(sm->lut_dim[0], sm->lut_dim[1], sm->lut_dim[2]);
  t.voxel_size = sm->voxel_size;
  t.voxel_size_inv = sm->voxel_size_inv;
  t.block_size = sm->block_size;
  t.block_size_inv = sm->block_size_inv;
  return t;
}
}  // namespace vgx

struct vgx_reg_s {
  vgx_ctx ctx = nullptr;
  vgx_submap reference = nullptr;
  vgx_submap reading = nullptr;
  vgx_reg_config cfg{};
  int64_t num_residuals = 0;
  uint64_t points_version = 0;  // PointSet::version of the reference points at construction
  // sampling mode state: a private engine when cfg.sampler_seed != 0, else the point set's
  vgx::SamplerEngine rng;
  // vgx_reg_evaluate_device_f32 in sampling mode only (it does not wait for its kernel, so it
  // cannot borrow a slot): own staging for the engine outputs, allocated at first use
  vgx::DeviceBuffer d_sample_raw;
  vgx::PinnedBuffer h_sample_raw;
  // Drop-in Evaluate calls arrive from several Ceres threads (pose_graph.cpp:96), each on its own
  // cost function; each call borrows one of the context's evaluation slots (Context::EvalSlot).
  std::mutex mu;                // two threads on the SAME cost function are serialised
  int draw_raw(uint32_t* out);  // 2 engine outputs per residual, drawn on the host
  vgx::SamplerEngine& engine(); // the stream this cost function samples from
  bool sampling() const { return cfg.sampling_ratio != -1.0f; }
  bool points_current() const;  // the reference submap still holds the points this was built on
  vgx::ConstraintDev describe() const;
  // Lifetime (vgx::lifetime_mu()): batches that list this cost function; vgx_reg_destroy while users > 0 is deferred to
  // the last vgx_reg_batch_destroy (ceres::Problem owns its cost functions for as long as it evaluates them).
  int users = 0;
  bool destroy_requested = false;
};

struct vgx_reg_batch_s {
  vgx_ctx ctx = nullptr;
  int32_t n = 0;
  int32_t n_global = 0;
  int layout = 0;                     // brick layout of every reading grid in the batch
  std::vector<vgx_reg> regs;
  std::vector<int32_t> node_pair;     // [n][2]
  std::vector<int32_t> global_index;  // [n]
  std::vector<int64_t> row_offset;    // [n+1]
  std::vector<vgx::Tile> tiles;
  // device arrays, typed at their uses (as<T>()); all go with the handle
  vgx::DeviceBuffer d_desc;           // ConstraintDev [n]
  vgx::DeviceBuffer d_pack;           // PosePack [n]
  vgx::UploadStage pack_stage;        // ... and their pinned staging, [n] per half
  vgx::DeviceBuffer d_tiles;          // Tile
  vgx::DeviceBuffer d_draw_tiles;     // Tile: the sampling constraints' tiles in the draw kernel's launch order
  int32_t n_draw_tiles = 0;
  vgx::DeviceBuffer d_drawn;          // float4; sampling: the point {x,y,z,d} every row uses in this evaluation (reg_gather_points_kernel)
  vgx::DeviceBuffer d_drawn_idx;      // int32 ... and its index in the point set (reg_draw_kernel)
  vgx::DeviceBuffer d_tile_dead;      // one BIT per materialising-pass tile, per launch: every chunk culled (rows are zeros)
  vgx::DeviceBuffer d_tile_first;     // int32 [n+1] first tile of each constraint
  vgx::DeviceBuffer d_partials;       // double [n_tiles][4 wavefronts][kPartialSize]
  vgx::DeviceBuffer d_normal;         // double [n][45] (internal, when caller passes none)
  bool normal_holds_blocks = false;   // d_normal holds the blocks of a vgx_reg_batch_evaluate_normal(d_normal == NULL): what
                                      // assemble / scatter_normal(NULL) may read (cleared by whatever else writes d_normal)
  vgx::PinnedBuffer h_normal;         // double [n][45]: staging of the host copies (normal_host / cost_host)
  vgx::DeviceBuffer d_node_pair;      // int32
  vgx::DeviceBuffer d_global_index;   // int32
  // fused pass: coarser tiles, and node -> incident (constraint<<1 | side) CSR
  std::vector<vgx::Tile> reduce_tiles;  // constraint-major; the device copy is re-ordered for launch at
                                        // the first evaluation (XCD-aware, make_xcd_order)
  std::vector<vgx::ConstraintDev> host_desc;
  std::vector<int32_t> host_tile_first;
  bool launch_order_made = false;
  bool launch_order_grouped = false, points_order_grouped = false;  // what make_xcd_order decided
  bool points_order_made = false;              // same, for the materialising pass's 1024-point tiles
  std::vector<int32_t> host_points_tile_first;
  vgx::DeviceBuffer d_reduce_tiles;   // Tile
  int32_t csr_nodes = 0;
  vgx::DeviceBuffer d_node_first;     // int32
  vgx::DeviceBuffer d_node_items;     // int32
  // sampling constraints (sampling_ratio != -1): one stream job per distinct engine, in order of
  // first appearance; the engine's constraints consume consecutive ranges of its stream in
  // constraint order, as successive Evaluate calls on one thread would (RCF:113-122)
  struct StreamJob {
    vgx::SamplerEngine* engine;
    int64_t offset;   // first word in d_raw
    int64_t count;    // words generated per evaluation
  };
  std::vector<StreamJob> stream_jobs;
  vgx::DeviceBuffer d_raw;         // uint32: all engine outputs of one evaluation
  vgx::DeviceBuffer d_stream_jobs; // device copy of {state*, out*, count} per job
  bool any_sampling = false;
  bool holds_regs = false;         // regs[*]->users were incremented (vgx_reg_batch_create succeeded)
  // vgx_reg_batch_evaluate_rows_f64 / _fetch_rows_f64: f64 rows the batch keeps itself (allocated at first use), and -- while
  // they are small enough (kRowsMirrorLimit) -- their pinned host mirror, filled by ONE device-to-host copy per evaluation
  vgx::DeviceBuffer d_rows[3];                       // double: residuals [R], jac_ref [R][4], jac_read [R][4]
  vgx::PinnedBuffer h_rows;                          // [R x 8][R x 32][R x 32], or empty (too large: fetches copy slices)
  bool rows_have[3] = {false, false, false};         // what the last rows evaluation produced
  bool rows_mirrored = false;                        // the mirror holds the last evaluation (its copy may still be in flight)
  // Lifetime (vgx::lifetime_mu()): pose graphs that were given this batch (vgx_pose_graph_set_registration);
  // vgx_reg_batch_destroy while users > 0 is deferred to the last of them letting go (a graph then refuses to solve).
  int users = 0;
  bool destroy_requested = false;
};

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
namespace vgx {
#ifndef VGX_TOOLING_LIBRARY
int set_error(vgx_ctx ctx, int code, const std::string& msg);
#else
inline int set_error(vgx_ctx ctx, int code, const std::string& msg);
#endif

// the one lock behind the users / destroy_requested fields of submaps and cost functions (vgx_context.hip)
std::mutex& lifetime_mu();

void set_global_error(const std::string& msg);

// The centre of voxel `idx` (one axis) of the block whose low corner on that axis is `origin` = (float)block_index *
// block_size, block_size = (float)vps * voxel_size: Block::computeCoordinatesFromLinearIndex [recalled], in f32, no
// contraction.  The one place this is written: the kVoxels points, the projected map and the layer clouds call it.
__host__ __device__ __forceinline__ float voxel_centre(float origin, int idx, float voxel_size) {
  return origin + ((float)idx + 0.5f) * voxel_size;
}

#define VGX_HIP(ctx, call)                                                      \
  do {                                                                          \
    hipError_t e__ = (call);                                                    \
    if (e__ != hipSuccess)                                                      \
      return vgx::set_error((ctx), VGX_ERR_HIP,                                 \
                            std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

// a failed device allocation of a product handle; `what`: "<product>: allocating <arrays>"
inline int alloc_error(vgx_ctx ctx, hipError_t e, const char* what) {
  (void)hipGetLastError();  // (clear the sticky out-of-memory status)
  return set_error(ctx, e == hipErrorOutOfMemory ? VGX_ERR_NOMEM : VGX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// a host array as a fresh device array of exactly `bytes` (blocking copy); nothing for bytes == 0: `buffer` stays empty
inline int upload_new(vgx_ctx ctx, DeviceBuffer& buffer, const void* src, size_t bytes) {
  buffer.release();
  if (bytes == 0) return VGX_OK;
  VGX_HIP(ctx, buffer.alloc(bytes));
  VGX_HIP(ctx, hipMemcpy(buffer.p, src, bytes, hipMemcpyHostToDevice));
  return VGX_OK;
}

// What vgx_connect.hip reads of a mesh handle (vgx_mesh_s lives in vgx_mesh.hip).  mesh_view: the caller holds
// mesh_mutex(M), except for `ctx`, which never changes.
struct MeshView {
  vgx_ctx ctx;
  bool holds_mesh;   // false after a generating call that failed
  bool has_colors;
  bool per_vertex;   // colors is [3 n_tris], one per soup vertex (vgx_*_generate_mesh_colored); else [n_tris]
  int64_t n_tris;
  const float* vertices;   // [n_tris][3][3]
  const float* normals;    // [n_tris][3]
  const uint32_t* colors;  // [n_tris] or [3 n_tris] bytes r g b a, or null
};
std::mutex& mesh_mutex(vgx_mesh M);
MeshView mesh_view(vgx_mesh M);

// vgx_eval.hip for vgx_cloud.hip (vgx_evaluate_layers_rmse_cloud): one evaluation left on the device.  eval_check
// refuses what vgx_evaluate_layers_rmse refuses (fn: the prefix of the message); eval_enqueue (the caller holds ctx->mu,
// the device is set) queues the passes of vgx_evaluate_layers_rmse on ctx->stream and leaves the totals and, when asked
// for, the error layer in `D` (freed with it); eval_details turns the totals, once on the host, into the details.
struct EvalTotals {
  double sum;
  float max_abs, min_abs;
  long long n_eval, n_ign, n_non, n_err_blocks;
};
struct EvalDevice {
  DeviceBuffer slot, has, pos, part, tot, tmp, ed, es, ebi;  // tot: EvalTotals; ed / es / ebi: [n_test] error blocks
};
int eval_check(const char* fn, vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode, const void* details);
int eval_enqueue(vgx_submap gt, vgx_submap test, int32_t layer, int32_t mode, bool want_index, bool want_distance, bool want_set,
                 EvalDevice& D);
void eval_details(const EvalTotals& tot, vgx_voxel_evaluation_details* details);

// kernels' launch wrappers implemented in the .hip files
#ifndef VGX_TOOLING_LIBRARY
int launch_brickify(vgx_submap sm, int which);
int build_block_lut(vgx_submap sm);
#else
inline int launch_brickify(vgx_submap sm, int which);
inline int build_block_lut(vgx_submap sm);
#endif
int build_chunk_bounds(vgx_ctx ctx, PointSet& ps);
// frees a point set's device arrays and leaves it empty (present = false) with a new version
void reset_point_set(PointSet& ps);
// sampler engines: make the host / the device copy the current one (ctx->mu held)
int engine_to_host(vgx_ctx ctx, SamplerEngine& e);
int engine_to_device(vgx_ctx ctx, SamplerEngine& e);
void make_pose_pack(const double ref_pose[4], const double read_pose[4], PosePack* out);
std::vector<Tile> make_tiles(int32_t constraint, int64_t n, int tile_points);
constexpr int kBlockThreads = 256;
// measured 4.38-4.41 / 4.35-4.37 / 4.67-4.68 ms per pass at 2 / 4 / 8 (config 3, a thread's point loads issued together:
// profiles/points_load_chain.txt; an earlier kernel, which issued them one after the other, measured 5.09-5.28 / 5.06-5.12 / 5.77-5.79)
constexpr int kPointsPerThread = 4;
constexpr int kTilePoints = kBlockThreads * kPointsPerThread;
}  // namespace vgx

// The library is built with -fvisibility=hidden: the C ABI of include/voxgraph_amd.h is what it exports -- plus these three
// hooks, C linkage like everything else, for libvoxgraph_amd_bench.so alone (csrc/bench/: scene generators, memory
// ceilings, the racing TSDF kernel's event log: test and benchmark tooling built from these same internal headers, kept
// out of the product library).  In no public header; vgx_context.hip defines them on vgx::set_error / launch_brickify /
// build_block_lut.
extern "C" {
VGX_API int vgx_internal_set_error(vgx_ctx ctx, int code, const char* msg);
VGX_API int vgx_internal_launch_brickify(vgx_submap sm, int which);
VGX_API int vgx_internal_build_block_lut(vgx_submap sm);
}
#ifdef VGX_TOOLING_LIBRARY
// inside the tooling library the internal names resolve to the hooks
namespace vgx {
inline int set_error(vgx_ctx ctx, int code, const std::string& msg) { return vgx_internal_set_error(ctx, code, msg.c_str()); }
inline int launch_brickify(vgx_submap sm, int which) { return vgx_internal_launch_brickify(sm, which); }
inline int build_block_lut(vgx_submap sm) { return vgx_internal_build_block_lut(sm); }
}  // namespace vgx
#endif

#endif
