// Map messages on the device: what voxgraph publishes at the end of every submap and every optimisation, and the
// receiving end.  voxblox::serializeLayerAsMsg / deserializeMsgToLayer [recalled] on the block words of
// vgx_mapfile_schema.h (SubmapServer::publishSubmapTsdf[AndEsdf] submap_server.cpp:83-105, ProjectedMapServer::
// publishProjectedMap projected_map_server.cpp:21-38), and the data bytes of the pcl::PointXYZI PointCloud2 of
// SubmapServer::publishSubmapSurfacePointcloud (submap_server.cpp:107-163).  The rules are stated in
// include/voxgraph_amd.h ("Map messages"), the kernels' resources and the measurement in DESIGN.md 18.
//
//   msg_serialize_kernel<SRC>   an interleaving copy: a thread owns 4 consecutive voxels, reads them as 16-byte vectors
//                               (packed {distance, weight} words + colours, or a submap's distance / weight / observed
//                               arrays) and writes their 12 (TSDF) or 8 (ESDF) consecutive words as 16-byte vectors
//   msg_surface_kernel          one registration point -> the 32 bytes of one pcl::PointXYZI
//   msg_deserialize_kernel      one workgroup per message block: the block's slot (allocated if absent), then its voxels
//                               replaced (kUpdate, kReset, a new block) or merged (kMerge into a present block)
// No atomics decide a position or a value; the only atomics are the block allocator's (get_or_allocate_block), which
// decide the slot of a new block, as after a scan.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "vgx_internal.h"
#include "vgx_mapfile_schema.h"
#include "vgx_tsdf_internal.h"

#pragma clang fp contract(off)

namespace vgx {

enum { kMsgSrcPacked = 0, kMsgSrcTsdf = 1, kMsgSrcEsdf = 2, kMsgSrcTsdfColor = 3 };  // (3: a submap with colours)

struct MsgSrc {
  const unsigned long long* words;  // packed: {distance (lo), weight (hi)}
  const uint32_t* rgba;             // packed, coloured submap TSDF: bytes r g b a
  const float* dist;                // submap TSDF / ESDF
  const void* seen;                 // submap TSDF: f32 weight; ESDF: u8 observed
  const int32_t* live_blocks;       // packed: the layer's allocation counter (device); null: every block of the grid
};

// Block<TsdfVoxel>::serializeToIntegers' colour word a | b << 8 | g << 16 | r << 24 of the stored bytes r g b a (r lowest)
__device__ __forceinline__ uint32_t msg_colour_word(uint32_t rgba) { return __builtin_bswap32(rgba); }

// Thread q owns the voxels 4 q .. 4 q + 3 (flat over blocks in slot order, linear-index order inside a block) and the
// words W * 4 q .. W * (4 q + 4) - 1 of the output: W / 4 * 4 consecutive 16-byte stores per thread, a wave's 64 threads
// one contiguous run of 3072 (TSDF) or 2048 (ESDF) bytes.
template <int SRC>
__global__ __launch_bounds__(256) void msg_serialize_kernel(MsgSrc s, size_t quads, size_t quads_per_block, uint4* __restrict__ out) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  size_t live = quads;
  if (SRC == kMsgSrcPacked && s.live_blocks) {
    const int32_t nb = *s.live_blocks;
    const size_t allocated = (size_t)(nb > 0 ? nb : 0) * quads_per_block;
    live = allocated < quads ? allocated : quads;
  }
  if (q >= live) return;
  if (SRC == kMsgSrcPacked) {
    const ulonglong2 a = reinterpret_cast<const ulonglong2*>(s.words)[2 * q];
    const ulonglong2 b = reinterpret_cast<const ulonglong2*>(s.words)[2 * q + 1];
    const uint4 c = reinterpret_cast<const uint4*>(s.rgba)[q];
    out[3 * q + 0] = make_uint4((uint32_t)a.x, (uint32_t)(a.x >> 32), msg_colour_word(c.x), (uint32_t)a.y);
    out[3 * q + 1] = make_uint4((uint32_t)(a.y >> 32), msg_colour_word(c.y), (uint32_t)b.x, (uint32_t)(b.x >> 32));
    out[3 * q + 2] = make_uint4(msg_colour_word(c.z), (uint32_t)b.y, (uint32_t)(b.y >> 32), msg_colour_word(c.w));
  } else if (SRC == kMsgSrcTsdf) {
    const uint4 d = reinterpret_cast<const uint4*>(s.dist)[q];
    const uint4 w = reinterpret_cast<const uint4*>(s.seen)[q];
    out[3 * q + 0] = make_uint4(d.x, w.x, 0u, d.y);
    out[3 * q + 1] = make_uint4(w.y, 0u, d.z, w.z);
    out[3 * q + 2] = make_uint4(0u, d.w, w.w, 0u);
  } else if (SRC == kMsgSrcTsdfColor) {
    const uint4 d = reinterpret_cast<const uint4*>(s.dist)[q];
    const uint4 w = reinterpret_cast<const uint4*>(s.seen)[q];
    const uint4 c = reinterpret_cast<const uint4*>(s.rgba)[q];
    out[3 * q + 0] = make_uint4(d.x, w.x, msg_colour_word(c.x), d.y);
    out[3 * q + 1] = make_uint4(w.y, msg_colour_word(c.y), d.z, w.z);
    out[3 * q + 2] = make_uint4(msg_colour_word(c.z), d.w, w.w, msg_colour_word(c.w));
  } else {
    const uint4 d = reinterpret_cast<const uint4*>(s.dist)[q];
    const uint32_t o = reinterpret_cast<const uint32_t*>(s.seen)[q];
    out[2 * q + 0] = make_uint4(d.x, (o & 0xffu) ? 1u : 0u, d.y, (o & 0xff00u) ? 1u : 0u);
    out[2 * q + 1] = make_uint4(d.z, (o & 0xff0000u) ? 1u : 0u, d.w, (o & 0xff000000u) ? 1u : 0u);
  }
}

struct MsgAffine {
  float m[12];  // row-major 3 x 4
  int32_t apply;
};

// pcl::PointXYZI as pcl::toROSMsg lays it out [recalled]: x y z data[3] = 1.0f | intensity, 12 bytes of padding
__global__ __launch_bounds__(256) void msg_surface_kernel(const float4* __restrict__ xyzd, const float* __restrict__ weight, size_t n,
                                                          MsgAffine T, uint4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = xyzd[i];
  float x = p.x, y = p.y, z = p.z;
  if (T.apply) {  // pcl::transformPoint: per row ((m0 x + m1 y) + m2 z) + t
    x = ((T.m[0] * p.x + T.m[1] * p.y) + T.m[2] * p.z) + T.m[3];
    y = ((T.m[4] * p.x + T.m[5] * p.y) + T.m[6] * p.z) + T.m[7];
    z = ((T.m[8] * p.x + T.m[9] * p.y) + T.m[10] * p.z) + T.m[11];
  }
  out[2 * i + 0] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0x3f800000u);
  out[2 * i + 1] = make_uint4(__float_as_uint(weight[i]), 0u, 0u, 0u);
}

// One workgroup per message block (the host has refused duplicates and reserved the box and the pool, so this
// workgroup alone touches its block).  MERGE: a block that was present gets mergeVoxelAIntoVoxelB(A = message, B = layer)
// per voxel; everything else is the message's voxel as it is.
template <int VPS, bool MERGE>
__global__ __launch_bounds__(256) void msg_deserialize_kernel(TsdfLayerDev L, const int32_t* __restrict__ block_index,
                                                              const uint4* __restrict__ words) {
  constexpr int VOX = VPS * VPS * VPS;
  constexpr int Q = VOX / 4;
  __shared__ int s_slot, s_present;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    const int bx = block_index[3 * (size_t)b], by = block_index[3 * (size_t)b + 1], bz = block_index[3 * (size_t)b + 2];
    const int rx = bx - L.lut_min[0], ry = by - L.lut_min[1], rz = bz - L.lut_min[2];
    int present = 0;
    if ((unsigned)rx < (unsigned)L.lut_dim[0] && (unsigned)ry < (unsigned)L.lut_dim[1] && (unsigned)rz < (unsigned)L.lut_dim[2])
      present = L.lut[rx + L.lut_dim[0] * (ry + L.lut_dim[1] * rz)] >= 0;
    const int slot = get_or_allocate_block(L, bx, by, bz);
    if (slot < 0) atomicAdd(L.dropped, (unsigned long long)VOX);  // (the host reserved the box and the pool: not reached)
    s_slot = slot;
    s_present = present;
  }
  __syncthreads();
  const int slot = s_slot;
  if (slot < 0) return;
  const bool merge = MERGE && s_present;
  const uint4* src = words + (size_t)b * (3 * Q);
  ulonglong2* vox = reinterpret_cast<ulonglong2*>(L.voxels + (size_t)slot * VOX);
  uint4* col = reinterpret_cast<uint4*>(L.rgba + (size_t)slot * VOX);
  for (int q = threadIdx.x; q < Q; q += 256) {
    const uint4 w0 = src[3 * q], w1 = src[3 * q + 1], w2 = src[3 * q + 2];
    const uint32_t db[4] = {w0.x, w0.w, w1.z, w2.y}, wb[4] = {w0.y, w1.x, w1.w, w2.z};
    uint32_t cb[4] = {msg_colour_word(w0.z), msg_colour_word(w1.y), msg_colour_word(w2.x), msg_colour_word(w2.w)};
    unsigned long long v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (unsigned long long)db[j] | ((unsigned long long)wb[j] << 32);
    if (merge) {
      const ulonglong2 o0 = vox[2 * q], o1 = vox[2 * q + 1];
      const uint4 oc4 = col[q];
      const unsigned long long old[4] = {o0.x, o0.y, o1.x, o1.y};
      const uint32_t oc[4] = {oc4.x, oc4.y, oc4.z, oc4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float da = __uint_as_float(db[j]), wa = __uint_as_float(wb[j]);
        const float dl = __uint_as_float((uint32_t)old[j]), wl = __uint_as_float((uint32_t)(old[j] >> 32));
        const float wn = wa + wl;
        if (wn > 0.0f) {
          v[j] = pack_voxel((da * wa + dl * wl) / wn, wn);
          cb[j] = blended_color(oc[j], cb[j], wl, wa);
        } else {
          v[j] = old[j];
          cb[j] = oc[j];
        }
      }
    }
    ulonglong2 a, c;
    a.x = v[0];
    a.y = v[1];
    c.x = v[2];
    c.y = v[3];
    vox[2 * q] = a;
    vox[2 * q + 1] = c;
    col[q] = make_uint4(cb[0], cb[1], cb[2], cb[3]);
  }
}

}  // namespace vgx

using namespace vgx;

struct vgx_map_msg_s {
  vgx_ctx ctx = nullptr;
  std::mutex mu;
  int32_t kind = VGX_MSG_NONE;  // what the handle holds now
  int64_t n = 0;                // blocks, or points
  int32_t words_per_voxel = 0, vps = 0;
  float voxel_size = 0.0f;
  // output, grown on demand to exactly what a message needs
  DeviceBuffer d_index;    // i32 [n][3] (layer messages)
  DeviceBuffer d_payload;  // u32 [n][vps^3 * words_per_voxel], or the cloud's 32 n bytes
};

namespace {

size_t msg_payload_bytes(const vgx_map_msg_s* M) {
  if (M->kind == VGX_MSG_SURFACE_CLOUD) return (size_t)M->n * 32;
  return (size_t)M->n * M->vps * M->vps * M->vps * M->words_per_voxel * 4;
}

int msg_check(vgx_ctx ctx, const char* fn, vgx_map_msg M) {
  if (!M) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": NULL message");
  if (M->ctx != ctx) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": the message belongs to another context");
  return VGX_OK;
}

// room for n items (caller holds M->mu); after a failure the handle holds nothing
int msg_reserve(vgx_map_msg M, size_t index_bytes, size_t payload_bytes) {
  M->kind = VGX_MSG_NONE;
  M->n = 0;
  hipError_t e = M->d_index.reserve(index_bytes);
  if (e == hipSuccess) e = M->d_payload.reserve(payload_bytes);
  return e == hipSuccess ? VGX_OK : alloc_error(M->ctx, e, "map message: allocating blocks");
}

// the interleaving copy of nb blocks on stream st, with the block indices; ends with the call's closing synchronisation
int msg_serialize(vgx_ctx ctx, hipStream_t st, int src, const MsgSrc& s, const int32_t* d_block_index, int32_t nb, int vps,
                  float voxel_size, vgx_map_msg M) {
  const int W = src == kMsgSrcEsdf ? vgx_schema::kEsdfWordsPerVoxel : vgx_schema::kTsdfWordsPerVoxel;
  const size_t vox = (size_t)vps * vps * vps;
  int rc = msg_reserve(M, (size_t)nb * 12, (size_t)nb * vox * W * 4);
  if (rc != VGX_OK) return rc;
  if (nb > 0) {
    const size_t quads = (size_t)nb * vox / 4;
    const unsigned grid = (unsigned)((quads + 255) / 256);
    uint4* out = M->d_payload.as<uint4>();
    VGX_HIP(ctx, hipMemcpyAsync(M->d_index.p, d_block_index, (size_t)nb * 12, hipMemcpyDeviceToDevice, st));
    if (src == kMsgSrcPacked) hipLaunchKernelGGL(msg_serialize_kernel<kMsgSrcPacked>, dim3(grid), dim3(256), 0, st, s, quads, vox / 4, out);
    else if (src == kMsgSrcTsdf) hipLaunchKernelGGL(msg_serialize_kernel<kMsgSrcTsdf>, dim3(grid), dim3(256), 0, st, s, quads, vox / 4, out);
    else if (src == kMsgSrcTsdfColor) hipLaunchKernelGGL(msg_serialize_kernel<kMsgSrcTsdfColor>, dim3(grid), dim3(256), 0, st, s, quads, vox / 4, out);
    else hipLaunchKernelGGL(msg_serialize_kernel<kMsgSrcEsdf>, dim3(grid), dim3(256), 0, st, s, quads, vox / 4, out);
    VGX_HIP(ctx, hipGetLastError());
    VGX_HIP(ctx, hipStreamSynchronize(st));
  }
  M->kind = src == kMsgSrcEsdf ? VGX_MSG_ESDF_LAYER : VGX_MSG_TSDF_LAYER;
  M->n = nb;
  M->words_per_voxel = W;
  M->vps = vps;
  M->voxel_size = voxel_size;
  return VGX_OK;
}

// vgx_tsdf_layer_deserialize[_msg] once the arguments have passed; block_index: host copy; d_index / d_words: device.
// The caller holds tsdf_mu, the device is set.
int msg_deserialize(vgx_tsdf_layer L, const char* fn, int32_t action, int32_t n, const int32_t* block_index, const int32_t* d_index,
                    const uint32_t* d_words) {
  vgx_ctx ctx = L->ctx;
  hipStream_t st = ctx->tsdf_stream;
  int32_t nb_now = 0;
  unsigned long long dropped = 0;
  int rc = tsdf_read_stats(L, &nb_now, &dropped);
  if (rc != VGX_OK) return rc;
  if (n > 0) {
    // room for every message block before any voxel is touched: the table covers their box, the pool holds them all
    int32_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = block_index[a];
    for (int32_t b = 1; b < n; ++b)
      for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(lo[a], block_index[3 * (size_t)b + a]);
        hi[a] = std::max(hi[a], block_index[3 * (size_t)b + a]);
      }
    const int64_t extra = action == VGX_MSG_ACTION_RESET ? std::max<int64_t>(0, (int64_t)n - nb_now) : (int64_t)n;
    rc = tsdf_reserve_blocks(L, lo, hi, extra);
    if (rc != VGX_OK) return rc;
  }
  const TsdfLayerDev& d = L->dev;
  const size_t vox = (size_t)d.vps * d.vps * d.vps;
  if (action == VGX_MSG_ACTION_RESET && nb_now > 0) {
    // the layer is emptied: a free table, a zero counter, and the used part of the pool back to fresh blocks (0, 0, 0)
    VGX_HIP(ctx, hipMemsetAsync(d.lut, 0xff, L->lut_cells * 4, st));
    VGX_HIP(ctx, hipMemsetAsync(d.voxels, 0, (size_t)nb_now * vox * 8, st));
    VGX_HIP(ctx, hipMemsetAsync(d.rgba, 0, (size_t)nb_now * vox * 4, st));
    VGX_HIP(ctx, hipMemsetAsync(d.n_blocks, 0, 4, st));
  }
  if (n > 0) {
    const bool merge = action == VGX_MSG_ACTION_MERGE;
    auto kernel = d.vps == 16 ? (merge ? msg_deserialize_kernel<16, true> : msg_deserialize_kernel<16, false>)
                              : (merge ? msg_deserialize_kernel<8, true> : msg_deserialize_kernel<8, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(256), 0, st, d, d_index, reinterpret_cast<const uint4*>(d_words));
    VGX_HIP(ctx, hipGetLastError());
  }
  rc = tsdf_read_stats(L, &nb_now, &dropped);  // (waits for the stream: the caller's arrays and the handle are free again)
  if (rc != VGX_OK) return rc;
  if (dropped != 0) return set_error(ctx, VGX_ERR_NOMEM, std::string(fn) + ": " + std::to_string(dropped) + " voxels dropped (allocation failed)");
  return VGX_OK;
}

// what both forms refuse from the numbers alone
int deserialize_check(vgx_tsdf_layer L, const char* fn, int32_t action, int32_t layer_type, double voxel_size, int32_t vps) {
  vgx_ctx ctx = L->ctx;
  auto fail = [ctx, fn](const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": " + msg); };
  if (action != VGX_MSG_ACTION_UPDATE && action != VGX_MSG_ACTION_MERGE && action != VGX_MSG_ACTION_RESET) return fail("unknown action");
  if (layer_type != VGX_EVAL_LAYER_TSDF) return fail("the layer type is not TSDF");
  if (vps != L->dev.vps) return fail("voxels_per_side differs from the layer's");
  // deserializeMsgToLayer's kVoxelSizeEpsilon = 1e-5 [recalled]
  if (!(std::fabs(voxel_size - (double)L->dev.voxel_size) <= 1e-5)) return fail("voxel_size differs from the layer's");
  return VGX_OK;
}

int has_duplicates(const int32_t* block_index, int32_t n) {
  std::vector<const int32_t*> p((size_t)n);
  for (int32_t b = 0; b < n; ++b) p[(size_t)b] = block_index + 3 * (size_t)b;
  auto less = [](const int32_t* a, const int32_t* b) { return std::lexicographical_compare(a, a + 3, b, b + 3); };
  std::sort(p.begin(), p.end(), less);
  for (int32_t b = 1; b < n; ++b)
    if (std::equal(p[(size_t)b], p[(size_t)b] + 3, p[(size_t)b - 1])) return 1;
  return 0;
}

}  // namespace

extern "C" {

int vgx_map_msg_create(vgx_ctx ctx, vgx_map_msg* out) {
  if (!ctx || !out) return set_error(ctx, VGX_ERR_INVALID, "vgx_map_msg_create: NULL argument");
  vgx_map_msg M = new vgx_map_msg_s;
  M->ctx = ctx;
  *out = M;
  return VGX_OK;
}

int vgx_map_msg_destroy(vgx_map_msg M) {
  if (!M) return VGX_ERR_INVALID;
  (void)hipSetDevice(M->ctx->device);
  delete M;
  return VGX_OK;
}

int vgx_map_msg_stats(vgx_map_msg M, int32_t* kind, int64_t* n, int32_t* words_per_voxel, int64_t* n_bytes) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  if (kind) *kind = M->kind;
  if (n) *n = M->n;
  if (words_per_voxel) *words_per_voxel = M->kind == VGX_MSG_TSDF_LAYER || M->kind == VGX_MSG_ESDF_LAYER ? M->words_per_voxel : 0;
  if (n_bytes) *n_bytes = M->kind == VGX_MSG_NONE ? 0 : (int64_t)msg_payload_bytes(M);
  return VGX_OK;
}

int vgx_map_msg_layer_geometry(vgx_map_msg M, float* voxel_size, int32_t* voxels_per_side) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  if (M->kind != VGX_MSG_TSDF_LAYER && M->kind != VGX_MSG_ESDF_LAYER)
    return set_error(M->ctx, VGX_ERR_INVALID, "vgx_map_msg_layer_geometry: the handle holds no layer message");
  if (voxel_size) *voxel_size = M->voxel_size;
  if (voxels_per_side) *voxels_per_side = M->vps;
  return VGX_OK;
}

int vgx_map_msg_device_pointers(vgx_map_msg M, const int32_t** block_index, const void** payload) {
  if (!M) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(M->mu);
  const bool any = M->kind != VGX_MSG_NONE && M->n > 0;
  if (block_index) *block_index = any && M->kind != VGX_MSG_SURFACE_CLOUD ? M->d_index.as<int32_t>() : nullptr;
  if (payload) *payload = any ? M->d_payload.p : nullptr;
  return VGX_OK;
}

int vgx_map_msg_download(vgx_map_msg M, int32_t* block_index, void* payload) {
  if (!M) return VGX_ERR_INVALID;
  vgx_ctx ctx = M->ctx;
  std::lock_guard<std::mutex> lk(M->mu);
  if (block_index && M->kind == VGX_MSG_SURFACE_CLOUD)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_map_msg_download: a surface cloud has no block indices");
  if (M->kind == VGX_MSG_NONE || M->n == 0) return VGX_OK;
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;  // (the message was complete when its producer returned, whichever stream made it)
  if (block_index) VGX_HIP(ctx, hipMemcpyAsync(block_index, M->d_index.p, (size_t)M->n * 12, hipMemcpyDeviceToHost, st));
  if (payload) VGX_HIP(ctx, hipMemcpyAsync(payload, M->d_payload.p, msg_payload_bytes(M), hipMemcpyDeviceToHost, st));
  VGX_HIP(ctx, hipStreamSynchronize(st));
  return VGX_OK;
}

int vgx_tsdf_layer_serialize(vgx_tsdf_layer L, vgx_map_msg M) {
  static const char* kFn = "vgx_tsdf_layer_serialize";
  if (!L) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL layer");
  vgx_ctx ctx = L->ctx;
  int rc = msg_check(ctx, kFn, M);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> msg_lk(M->mu);
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  const TsdfLayerDev& d = L->dev;
  if (d.vps != 8 && d.vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + ": voxels_per_side must be 8 or 16");
  // the block total (first synchronisation: behind the scans and merges queued on the TSDF stream); the kernel reads the
  // allocation counter on the device all the same and never goes past it
  int32_t nb = 0;
  unsigned long long dropped = 0;
  rc = tsdf_read_stats(L, &nb, &dropped);
  if (rc != VGX_OK) return rc;
  MsgSrc s{};
  s.words = d.voxels;
  s.rgba = d.rgba;
  s.live_blocks = d.n_blocks;
  return msg_serialize(ctx, ctx->tsdf_stream, kMsgSrcPacked, s, d.block_index, nb, d.vps, d.voxel_size, M);
}

int vgx_submap_serialize_layer(vgx_submap sm, int32_t layer, vgx_map_msg M) {
  static const char* kFn = "vgx_submap_serialize_layer";
  if (!sm) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL submap");
  vgx_ctx ctx = sm->ctx;
  int rc = msg_check(ctx, kFn, M);
  if (rc != VGX_OK) return rc;
  if (layer != VGX_EVAL_LAYER_ESDF && layer != VGX_EVAL_LAYER_TSDF)
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": layer is neither ESDF nor TSDF");
  const bool tsdf = layer == VGX_EVAL_LAYER_TSDF;
  if (sm->n_blocks > 0 && (tsdf ? (!sm->d_tsdf_distance || !sm->d_tsdf_weight) : (!sm->d_esdf_distance || !sm->d_esdf_observed)))
    return set_error(ctx, VGX_ERR_INVALID,
                     std::string(kFn) + (tsdf ? ": TSDF" : ": ESDF") + " layer not resident (released, or never generated)");
  if (sm->vps != 8 && sm->vps != 16) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + ": voxels_per_side must be 8 or 16");
  std::lock_guard<std::mutex> msg_lk(M->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  MsgSrc s{};
  s.dist = tsdf ? sm->d_tsdf_distance : sm->d_esdf_distance;
  s.seen = tsdf ? (const void*)sm->d_tsdf_weight : (const void*)sm->d_esdf_observed;
  s.rgba = tsdf ? sm->d_tsdf_rgba : nullptr;
  return msg_serialize(ctx, ctx->stream, tsdf ? (s.rgba ? kMsgSrcTsdfColor : kMsgSrcTsdf) : kMsgSrcEsdf, s, sm->d_block_index, sm->n_blocks, sm->vps, sm->voxel_size, M);
}

int vgx_submap_surface_msg(vgx_submap sm, int32_t point_type, const float* T, vgx_map_msg M) {
  static const char* kFn = "vgx_submap_surface_msg";
  if (!sm) return set_error(M ? M->ctx : nullptr, VGX_ERR_INVALID, std::string(kFn) + ": NULL submap");
  vgx_ctx ctx = sm->ctx;
  int rc = msg_check(ctx, kFn, M);
  if (rc != VGX_OK) return rc;
  if (point_type != VGX_POINTS_ISOSURFACE && point_type != VGX_POINTS_VOXELS)
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": unknown point type");
  MsgAffine A{};
  if (T) {
    for (int k = 0; k < 12; ++k) {
      if (!std::isfinite(T[k])) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": a transform entry is not finite");
      A.m[k] = T[k];
    }
    A.apply = 1;
  }
  std::lock_guard<std::mutex> msg_lk(M->mu);
  std::lock_guard<std::mutex> reg_lk(ctx->mu);
  const PointSet& ps = sm->points[point_type];
  if (!ps.present) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": no such point set (never extracted or uploaded)");
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  rc = msg_reserve(M, 0, (size_t)ps.n * 32);
  if (rc != VGX_OK) return rc;
  if (ps.n > 0) {
    hipLaunchKernelGGL(msg_surface_kernel, dim3((unsigned)((ps.n + 255) / 256)), dim3(256), 0, ctx->stream, ps.d_xyzd, ps.d_weight,
                       (size_t)ps.n, A, M->d_payload.as<uint4>());
    VGX_HIP(ctx, hipGetLastError());
    VGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  M->kind = VGX_MSG_SURFACE_CLOUD;
  M->n = ps.n;
  M->words_per_voxel = 0;
  M->vps = 0;
  M->voxel_size = 0.0f;
  return VGX_OK;
}

int vgx_tsdf_layer_deserialize(vgx_tsdf_layer L, int32_t action, int32_t layer_type, double voxel_size, int32_t vps, int32_t n,
                               const int32_t* block_index, const uint32_t* words, int64_t n_words) {
  static const char* kFn = "vgx_tsdf_layer_deserialize";
  if (!L) return VGX_ERR_INVALID;
  vgx_ctx ctx = L->ctx;
  int rc = deserialize_check(L, kFn, action, layer_type, voxel_size, vps);
  if (rc != VGX_OK) return rc;
  auto fail = [ctx](const std::string& msg) { return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": " + msg); };
  if (n < 0) return fail("n_blocks < 0");
  if (n_words != (int64_t)n * vps * vps * vps * vgx_schema::kTsdfWordsPerVoxel) return fail("the words' length is not n_blocks * voxels_per_side^3 * 3");
  if (n > 0 && (!block_index || !words)) return fail("NULL arrays with n_blocks > 0");
  if (has_duplicates(block_index, n)) return fail("a block index appears twice");
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  DeviceBuffer d_index, d_words;
  if (n > 0) {
    hipError_t e = d_index.alloc((size_t)n * 12);
    if (e == hipSuccess) e = d_words.alloc((size_t)n_words * 4);
    if (e != hipSuccess) return alloc_error(ctx, e, "vgx_tsdf_layer_deserialize: allocating the message");
    VGX_HIP(ctx, hipMemcpyAsync(d_index.p, block_index, (size_t)n * 12, hipMemcpyHostToDevice, ctx->tsdf_stream));
    VGX_HIP(ctx, hipMemcpyAsync(d_words.p, words, (size_t)n_words * 4, hipMemcpyHostToDevice, ctx->tsdf_stream));
  }
  return msg_deserialize(L, kFn, action, n, block_index, d_index.as<int32_t>(), d_words.as<uint32_t>());
}

int vgx_tsdf_layer_deserialize_msg(vgx_tsdf_layer L, int32_t action, vgx_map_msg M) {
  static const char* kFn = "vgx_tsdf_layer_deserialize_msg";
  if (!L) return VGX_ERR_INVALID;
  vgx_ctx ctx = L->ctx;
  int rc = msg_check(ctx, kFn, M);
  if (rc != VGX_OK) return rc;
  std::lock_guard<std::mutex> msg_lk(M->mu);
  if (M->kind != VGX_MSG_TSDF_LAYER && M->kind != VGX_MSG_ESDF_LAYER)
    return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": the handle holds no layer message");
  rc = deserialize_check(L, kFn, action, M->kind == VGX_MSG_TSDF_LAYER ? VGX_EVAL_LAYER_TSDF : VGX_EVAL_LAYER_ESDF, (double)M->voxel_size,
                         M->vps);
  if (rc != VGX_OK) return rc;
  if (M->n > INT32_MAX) return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(kFn) + ": more than 2^31 blocks");
  const int32_t n = (int32_t)M->n;
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  // the block indices alone come to the host (the box to reserve); the words stay where they are
  std::vector<int32_t> block_index(3 * (size_t)n);
  if (n > 0) VGX_HIP(ctx, hipMemcpy(block_index.data(), M->d_index.p, (size_t)n * 12, hipMemcpyDeviceToHost));
  if (has_duplicates(block_index.data(), n)) return set_error(ctx, VGX_ERR_INVALID, std::string(kFn) + ": a block index appears twice");
  return msg_deserialize(L, kFn, action, n, block_index.data(), M->d_index.as<int32_t>(), M->d_payload.as<uint32_t>());
}

}  // extern "C"
