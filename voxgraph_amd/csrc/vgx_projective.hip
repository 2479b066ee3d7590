// Projective depth-image integration (include/voxgraph_amd.h, "Projective depth-image integration"): every
// voxel of the camera's frustum projects itself into the depth image, reads ONE depth and folds one update into itself.
// A gather: a lane owns its voxels, so no atomic touches a voxel, nothing is sorted and no approximate set is asked --
// the layer is the same bit for bit on every run by construction.
//
// ONE kernel per frame: the block walk of vgx_projective_kernel.h (shared with the LiDAR range-image integrator,
// vgx_range_image.hip) instantiated for the pinhole frame below.  The host computes the candidate block box (vgx_tsdf_projective_box, f64) and makes room for it
// (tsdf_reserve_blocks: its read of the exact block count is the frame's one host synchronisation); a workgroup of 512
// lanes takes the candidate block of its ticket (TileChain, vgx_tsdf_internal.h: tickets are given in the order the
// workgroups start, candidate = ticket, ascending (z, y, x)), every lane walks vps^3 / 512 voxels (1 or 8), one lane per
// voxel at a time with neighbouring lanes on neighbouring x -- neighbouring pixels, through the ordinary cache path.  The
// old voxel is loaded only where the frame updates it.  A block-wide vote says whether an ABSENT block has a voxel
// that changes; such a block takes the pool slot
//     (blocks the layer held before the frame) + (needed absent candidates before it)
// -- the second term is chain_exclusive_sum over the tiles before it, the prefix sum inside the launch that the scan
// decode uses -- and only then are its voxels written (into pool memory that is zero: a fresh block): of an absent
// block the first pass keeps one bit per voxel, and the voxels that change are formed a second time once the slot is
// known (holding a lane's voxels' results across the vote spilled).  The last candidate leaves the new block count.  No
// atomicAdd decides a slot: block order is a function of the input alone.
//
// Whole blocks are rejected early where their bounding sphere (plus a margin far above the f32 rounding of the per-voxel
// arithmetic) lies behind the camera, beyond the far gate or outside one of the image's four side planes: no voxel of such
// a block can find a pixel.  A rejected block still takes its place in the chain (it reports "not needed").
#include <cmath>
#include <cstring>
#include <string>

#include "vgx_projective_kernel.h"
#include "vgx_depth_image.h"

#pragma clang fp contract(off)

namespace vgx {

constexpr size_t kProjStageBytes = 1u << 20;  // one pinned staging piece of the host form

struct ProjFrame : ProjFrameBase {
  DepthImage img;  // depth, color, row_step, color_row_step, color_kind, unit, min_z, max_z
  uint32_t width, height;
  float fx, fy, cx, cy;  // (float) of the camera's
  float z_far;            // no voxel beyond it can be updated (early reject only)
  int32_t reject;         // side planes usable (fx, fy > 0)
};

// the depth-image frame, as the generic block walk (vgx_projective_kernel.h) asks for it
template <int ENC, bool ELEMENTS>
struct PinholeFrame : ProjFrame {
  // can any voxel of block (bx, by, bz) find a pixel?  (conservative: true when in doubt)
  __device__ __forceinline__ bool block_in_view(float block_size, int bx, int by, int bz) const {
    const ProjFrame& f = *this;
    float x, y, z;
    const float r = block_sphere(f, block_size, bx, by, bz, x, y, z);
    if (!(z + r > 0.0f)) return false;      // z > 0 fails for every voxel
    if (z - r > f.z_far) return false;      // beyond the depth gate and the ray length, truncation included
    if (!f.reject) return true;
    const float w = (float)f.width, h = (float)f.height;
    const float l0 = f.cx + 0.5f, r0 = l0 - w, t0 = f.cy + 0.5f, b0 = t0 - h;
    // 0 <= (x / z) fx + cx + 0.5 fails for every point of the sphere with z > 0 when the sphere lies wholly on the
    // negative side of the plane fx x + (cx + 0.5) z = 0; the other three alike
    if (f.fx * x + l0 * z < -r * sqrtf(f.fx * f.fx + l0 * l0)) return false;
    if (f.fx * x + r0 * z > r * sqrtf(f.fx * f.fx + r0 * r0)) return false;
    if (f.fy * y + t0 * z < -r * sqrtf(f.fy * f.fy + t0 * t0)) return false;
    if (f.fy * y + b0 * z > r * sqrtf(f.fy * f.fy + b0 * b0)) return false;
    return true;
  }

  // What the frame does to the voxel (vx, vy, vz): false = no update; else the update's sdf, weight and colour, and
  // kind = 0 inside the truncation band or behind the surface, 1 carved, 2 cleared.  The rules of the header, in its order.
  __device__ __forceinline__ bool term(const vgx_tsdf_config& c, float vs, int vx, int vy, int vz, float& sdf, float& uw,
                                       uint32_t& color, int& kind) const {
    const ProjFrame& f = *this;
    const float gx = ((float)vx + 0.5f) * vs, gy = ((float)vy + 0.5f) * vs, gz = ((float)vz + 0.5f) * vs;
    float x, y, z;
    to_camera(f, gx, gy, gz, x, y, z);
    if (!(z > 0.0f)) return false;
    const float uf = (x / z) * f.fx + f.cx, vf = (y / z) * f.fy + f.cy;
    const float ua = uf + 0.5f, va = vf + 0.5f;
    if (!(ua >= 0.0f && ua < (float)f.width && va >= 0.0f && va < (float)f.height)) return false;
    const uint32_t ui = (uint32_t)floorf(ua), vi = (uint32_t)floorf(va);
    const float d = depth_z<ENC, ELEMENTS>(f.img, f.img.depth + (size_t)vi * f.img.row_step, ui);
    if (!(d > 0.0f && d < INFINITY)) return false;            // the decode's rule 1
    if (!(d >= f.img.min_z && d <= f.img.max_z)) return false;  // ... and 2
    const float trunc = c.default_truncation_distance;
    const float r_v = norm3(x, y, z);
    const float s = r_v / z;
    const float r_s = d * s;
    sdf = (d - z) * s;
    kind = 0;
    if (r_s < c.min_ray_length_m) return false;
    if (r_s > c.max_ray_length_m) {
      if (!(c.allow_clear && c.voxel_carving_enabled && r_v + trunc <= c.max_ray_length_m)) return false;
      sdf = c.max_ray_length_m - r_v;
      kind = 2;
    } else {
      if (sdf < -trunc) return false;
      if (sdf > trunc) {
        if (!c.voxel_carving_enabled) return false;
        kind = 1;
      }
    }
    uw = c.use_const_weight ? 1.0f : 1.0f / (d * d);
    if (c.use_weight_dropoff && sdf < -vs) {  // update_term's drop-off (vgx_tsdf_det.hip)
      uw = uw * (trunc + sdf) / (trunc - vs);
      uw = fmaxf(uw, 0.0f);
    }
    color = f.img.color_kind == VGX_IMAGE_COLOR_NONE ? 0xffffffffu : depth_colour(f.img, ui, vi);
    return true;
  }
};

// The candidate block box, f64 throughout: the axis-aligned box (layer frame) of the camera centre and of the points
// where the four image-corner rays -- through (-0.5, -0.5), (width - 0.5, -0.5), (-0.5, height - 0.5), (width - 0.5,
// height - 0.5), the corners of the area whose pixels can be looked up -- reach the z-depth `reach`.
int projective_box(const vgx_depth_image_layout& l, const vgx_depth_camera& cam, const vgx_tsdf_config& c, const float T[7],
                   float voxel_size, int32_t vps, int32_t lo[3], int32_t hi[3], std::string* why) {
  auto fail = [why](int code, const char* msg) {
    if (why) *why = msg;
    return code;
  };
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(T[k])) return fail(VGX_ERR_INVALID, "T_G_C is not finite");
  if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size) || (vps != 8 && vps != 16))
    return fail(VGX_ERR_INVALID, "voxel_size is not positive or voxels_per_side is not 8 or 16");
  // ((float)width is exact below 2^24: the f32 pixel test then never lets a column or row past the image's edge)
  if (l.width >= (1u << 24) || l.height >= (1u << 24)) return fail(VGX_ERR_UNSUPPORTED, "width or height is 2^24 or more");
  const double trunc = (double)c.default_truncation_distance;
  const double reach = std::fmin((double)cam.max_depth_m, (double)c.max_ray_length_m) + trunc;
  if (!std::isfinite(reach) || !(reach > 0.0)) return fail(VGX_ERR_UNSUPPORTED, "the depth gate and max_ray_length_m are both unbounded");
  const double bs = (double)voxel_size * (double)vps;
  const double qw = T[0], qx = T[1], qy = T[2], qz = T[3];
  double mn[3] = {(double)T[4], (double)T[5], (double)T[6]}, mx[3] = {mn[0], mn[1], mn[2]};
  for (int corner = 0; corner < 4; ++corner) {
    const double u = (corner & 1) ? (double)l.width - 0.5 : -0.5, v = (corner & 2) ? (double)l.height - 0.5 : -0.5;
    const double px = ((u - cam.cx) / cam.fx) * reach, py = ((v - cam.cy) / cam.fy) * reach, pz = reach;
    double uvx = qy * pz - qz * py, uvy = qz * px - qx * pz, uvz = qx * py - qy * px;
    uvx += uvx; uvy += uvy; uvz += uvz;
    const double ccx = qy * uvz - qz * uvy, ccy = qz * uvx - qx * uvz, ccz = qx * uvy - qy * uvx;
    const double g[3] = {(px + qw * uvx + ccx) + (double)T[4], (py + qw * uvy + ccy) + (double)T[5], (pz + qw * uvz + ccz) + (double)T[6]};
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::fmin(mn[a], g[a]);
      mx[a] = std::fmax(mx[a], g[a]);
    }
  }
  for (int a = 0; a < 3; ++a) {
    const double flo = std::floor(mn[a] / bs) - 1.0, fhi = std::floor(mx[a] / bs) + 1.0;
    if (!(flo > -1073741824.0 && fhi < 1073741824.0)) return fail(VGX_ERR_UNSUPPORTED, "the candidate box exceeds +-2^30 blocks");
    lo[a] = (int32_t)flo;
    hi[a] = (int32_t)fhi;
  }
  return VGX_OK;
}

int projective_begin(const char* fn, vgx_tsdf_integrator I, const int32_t lo[3], const int32_t hi[3], ProjFrameBase* f) {
  vgx_ctx ctx = I->ctx;
  vgx_tsdf_layer L = I->layer;
  const int64_t nx = (int64_t)hi[0] - lo[0] + 1, ny = (int64_t)hi[1] - lo[1] + 1, nz = (int64_t)hi[2] - lo[2] + 1;
  if (nx * ny > kProjMaxCandidates || nx * ny * nz > kProjMaxCandidates)
    return set_error(ctx, VGX_ERR_UNSUPPORTED, std::string(fn) + ": the candidate box holds more than 2^24 blocks");
  const int64_t candidates = nx * ny * nz;
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->tsdf_stream;
  // room for every candidate; waits for the stream and reads the exact block count: the frame's one host synchronisation
  const int rc = tsdf_reserve_blocks(L, lo, hi, candidates);
  if (rc != VGX_OK) return rc;
  const int32_t base_blocks = (int32_t)L->known_blocks;  // (exact: tsdf_reserve_blocks has just read it behind everything queued)
  // the control words and one chain word per candidate
  if (!I->d_proj_ctl.p) {
    const hipError_t e = I->d_proj_ctl.alloc(kProjCtlWords * 8);
    if (e != hipSuccess) return alloc_error(ctx, e, "projective integration: allocating counters");
    VGX_HIP(ctx, hipMemsetAsync(I->d_proj_ctl.p, 0, kProjCtlWords * 8, st));
    I->proj_clock.tickets = 0;
  }
  if ((size_t)candidates * 8 > I->d_proj_state.bytes) {
    VGX_HIP(ctx, hipStreamSynchronize(st));
    const hipError_t e = I->d_proj_state.reserve((size_t)candidates * 8, 0, true);
    if (e != hipSuccess) return alloc_error(ctx, e, "projective integration: allocating tile words");
    VGX_HIP(ctx, hipMemsetAsync(I->d_proj_state.p, 0, I->d_proj_state.bytes, st));  // (epoch 0: no launch's tag)
  }
  for (int a = 0; a < 3; ++a) f->lo[a] = lo[a];
  f->nx = (int32_t)nx;
  f->ny = (int32_t)ny;
  f->tiles = (uint32_t)candidates;
  f->base_blocks = base_blocks;
  return VGX_OK;
}

int projective_chain(vgx_tsdf_integrator I, const ProjFrameBase& f, TileChain* chain) {
  vgx_ctx ctx = I->ctx;
  unsigned long long* ctl = I->d_proj_ctl.as<unsigned long long>();
  VGX_HIP(ctx, hipMemsetAsync(ctl + kProjNew, 0, 8 * (kProjCtlWords - kProjNew), ctx->tsdf_stream));
  ChainTake t;
  VGX_HIP(ctx, chain_take(&I->proj_clock, f.tiles, I->d_proj_state, ctx->tsdf_stream, &t));
  chain->state = I->d_proj_state.as<unsigned long long>();
  chain->epoch = t.epoch;
  chain->ticket = ctl + kProjTicket;
  chain->ticket_base = t.ticket_base;
  chain->error = ctl + kProjError;
  return VGX_OK;
}

int projective_end(const char* fn, vgx_tsdf_integrator I, const ProjFrameBase& f, vgx_projective_counts* counts) {
  vgx_ctx ctx = I->ctx;
  hipStream_t st = ctx->tsdf_stream;
  unsigned long long* ctl = I->d_proj_ctl.as<unsigned long long>();
  VGX_HIP(ctx, hipGetLastError());
  tsdf_note_allocations(I->layer, (int64_t)f.tiles);
  if (counts) {
    unsigned long long back[kProjCtlWords - kProjError] = {};
    VGX_HIP(ctx, hipMemcpyAsync(back, ctl + kProjError, sizeof(back), hipMemcpyDeviceToHost, st));
    VGX_HIP(ctx, hipStreamSynchronize(st));
    if (back[0] != 0) {
      (void)hipMemsetAsync(ctl + kProjError, 0, 8, st);
      return set_error(ctx, VGX_ERR_HIP, std::string(fn) + ": a candidate block never reported (internal error)");
    }
    if (back[kProjDropped - kProjError] != 0)
      return set_error(ctx, VGX_ERR_NOMEM, std::string(fn) + ": voxel updates were dropped (no room for a block)");
    vgx_projective_counts out{};
    out.n_candidate_blocks = (int64_t)f.tiles;
    out.n_new_blocks = (int64_t)back[kProjNew - kProjError];
    out.n_updates = (int64_t)back[kProjUpdates - kProjError];
    out.n_carved = (int64_t)back[kProjCarved - kProjError];
    out.n_cleared = (int64_t)back[kProjCleared - kProjError];
    *counts = out;
  }
  return VGX_OK;
}

}  // namespace vgx

using namespace vgx;

namespace {

template <int ENC, bool ELEMENTS>
void pinhole_launch(hipStream_t st, const TsdfLayerDev& L, const vgx_tsdf_config& c, const ProjFrame& f, const TileChain& chain,
                    unsigned long long* ctl) {
  PinholeFrame<ENC, ELEMENTS> frame;
  static_cast<ProjFrame&>(frame) = f;
  projective_launch(st, L, c, frame, chain, ctl);
}

// the images' bytes into the integrator's image buffer through its pinned staging halves (pieces of 1 MiB, filled in turn)
int upload_image(vgx_tsdf_integrator I, const void* data, size_t bytes, size_t dst) {
  vgx_ctx ctx = I->ctx;
  hipStream_t st = ctx->tsdf_stream;
  if (I->stage.bytes() < kProjStageBytes) {
    VGX_HIP(ctx, hipStreamSynchronize(st));  // (a queued upload may still read the halves)
    if (I->stage.reserve(kProjStageBytes) != hipSuccess) (void)hipGetLastError();  // no pinned memory to be had: the pageable path below
  }
  if (I->stage.bytes() < kProjStageBytes) {
    VGX_HIP(ctx, hipMemcpyAsync(I->d_image.as<char>() + dst, data, bytes, hipMemcpyHostToDevice, st));
    VGX_HIP(ctx, hipStreamSynchronize(st));  // the caller's bytes are theirs again when the call returns
    return VGX_OK;
  }
  const size_t piece_max = I->stage.bytes();
  for (size_t at = 0; at < bytes; at += piece_max) {
    const size_t piece = std::min(piece_max, bytes - at);
    int k = 0;
    hipError_t waited = hipSuccess;
    void* h = I->stage.next(&k, &waited);
    VGX_HIP(ctx, waited);
    std::memcpy(h, static_cast<const char*>(data) + at, piece);
    VGX_HIP(ctx, hipMemcpyAsync(I->d_image.as<char>() + dst + at, h, piece, hipMemcpyHostToDevice, st));
    VGX_HIP(ctx, I->stage.record(k, st));
  }
  return VGX_OK;
}

int integrate_depth_image(const char* fn, vgx_tsdf_integrator I, const float T[7], const vgx_depth_image_layout* l,
                          const vgx_depth_camera* cam, const void* depth, int64_t depth_n_bytes, const void* color,
                          int64_t color_n_bytes, vgx_projective_counts* counts, bool on_device) {
  // the frame is checked first: what vgx_depth_image_check refuses is refused with its code whatever else is wrong
  std::string why;
  int rc = depth_image_check(l, cam, depth_n_bytes, color_n_bytes, &why);
  if (!I) return rc != VGX_OK ? rc : VGX_ERR_INVALID;
  vgx_ctx ctx = I->ctx;
  if (rc == VGX_OK && !T) {
    rc = VGX_ERR_INVALID;
    why = "NULL pose";
  }
  const size_t n = rc == VGX_OK ? (size_t)l->width * l->height : 0;
  if (rc == VGX_OK && n > 0 && !depth) {
    rc = VGX_ERR_INVALID;
    why = "NULL depth image";
  }
  if (rc == VGX_OK && n > 0 && l->color_kind != VGX_IMAGE_COLOR_NONE && !color) {
    rc = VGX_ERR_INVALID;
    why = "NULL colour image";
  }
  if (rc != VGX_OK) return set_error(ctx, rc, std::string(fn) + ": " + why);
  std::lock_guard<std::mutex> own(I->mu);
  std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
  if (!I->layer) return set_error(ctx, VGX_ERR_INVALID, std::string(fn) + ": no layer set");
  vgx_tsdf_layer L = I->layer;
  const vgx_tsdf_config& c = I->dev.cfg;
  vgx_projective_counts out{};
  if (n == 0) {
    if (counts) *counts = out;
    return VGX_OK;
  }
  int32_t lo[3], hi[3];
  rc = projective_box(*l, *cam, c, T, L->dev.voxel_size, L->dev.vps, lo, hi, &why);
  if (rc != VGX_OK) return set_error(ctx, rc, std::string(fn) + ": " + why);
  ProjFrame f{};
  rc = projective_begin(fn, I, lo, hi, &f);
  if (rc != VGX_OK) return rc;
  hipStream_t st = ctx->tsdf_stream;
  const bool colour = l->color_kind != VGX_IMAGE_COLOR_NONE;
  const uint8_t* d_depth = static_cast<const uint8_t*>(depth);
  const uint8_t* d_color = colour ? static_cast<const uint8_t*>(color) : nullptr;
  if (!on_device) {
    // both images into one buffer, the colour image at the next multiple of 16 bytes
    const size_t bytes = (size_t)(l->height - 1) * l->row_step + (size_t)l->width * depth_bpp(l->encoding);
    const size_t cbytes = colour ? (size_t)(l->height - 1) * l->color_row_step + (size_t)l->width * colour_bpp(l->color_kind) : 0;
    const size_t cat = (bytes + 15) & ~(size_t)15;
    if (cat + cbytes > I->d_image.bytes) {
      VGX_HIP(ctx, hipStreamSynchronize(st));
      const hipError_t e = I->d_image.alloc(cat + cbytes);
      if (e != hipSuccess) return alloc_error(ctx, e, "projective integration: allocating the images");
    }
    rc = upload_image(I, depth, bytes, 0);
    if (rc == VGX_OK && colour) rc = upload_image(I, color, cbytes, cat);
    if (rc != VGX_OK) return rc;
    d_depth = I->d_image.as<uint8_t>();
    d_color = colour ? d_depth + cat : nullptr;
  }
  f.img.depth = d_depth;
  f.img.color = d_color;
  f.img.row_step = l->row_step;
  f.img.color_row_step = colour ? l->color_row_step : 0u;
  f.img.color_kind = l->color_kind;
  f.img.unit = cam->depth_unit_m;
  f.img.min_z = cam->min_depth_m;
  f.img.max_z = cam->max_depth_m;
  f.width = l->width;
  f.height = l->height;
  f.fx = (float)cam->fx;
  f.fy = (float)cam->fy;
  f.cx = (float)cam->cx;
  f.cy = (float)cam->cy;
  f.qw = T[0]; f.qx = T[1]; f.qy = T[2]; f.qz = T[3];
  f.tx = T[4]; f.ty = T[5]; f.tz = T[6];
  f.z_far = std::fmin(cam->max_depth_m, c.max_ray_length_m) + c.default_truncation_distance;
  f.reject = f.fx > 0.0f && f.fy > 0.0f && std::isfinite(f.fx) && std::isfinite(f.fy);
  TileChain chain;
  rc = projective_chain(I, f, &chain);
  if (rc != VGX_OK) return rc;
  unsigned long long* ctl = I->d_proj_ctl.as<unsigned long long>();
  const bool sixteen = l->encoding == VGX_DEPTH_16UC1;
  const bool elements = ((uintptr_t)d_depth | l->row_step) % (sixteen ? 2u : 4u) == 0;
  if (sixteen) {
    if (elements) pinhole_launch<VGX_DEPTH_16UC1, true>(st, L->dev, c, f, chain, ctl);
    else pinhole_launch<VGX_DEPTH_16UC1, false>(st, L->dev, c, f, chain, ctl);
  } else {
    if (elements) pinhole_launch<VGX_DEPTH_32FC1, true>(st, L->dev, c, f, chain, ctl);
    else pinhole_launch<VGX_DEPTH_32FC1, false>(st, L->dev, c, f, chain, ctl);
  }
  return projective_end(fn, I, f, counts);
}

}  // namespace

extern "C" {

int vgx_tsdf_integrate_depth_image(vgx_tsdf_integrator I, const float T_G_C[7], const vgx_depth_image_layout* layout,
                                   const vgx_depth_camera* camera, const void* depth, int64_t depth_n_bytes, const void* color,
                                   int64_t color_n_bytes, vgx_projective_counts* counts) {
  return integrate_depth_image("vgx_tsdf_integrate_depth_image", I, T_G_C, layout, camera, depth, depth_n_bytes, color, color_n_bytes,
                               counts, false);
}

int vgx_tsdf_integrate_depth_image_device(vgx_tsdf_integrator I, const float T_G_C[7], const vgx_depth_image_layout* layout,
                                          const vgx_depth_camera* camera, const void* d_depth, int64_t depth_n_bytes,
                                          const void* d_color, int64_t color_n_bytes, vgx_projective_counts* counts) {
  return integrate_depth_image("vgx_tsdf_integrate_depth_image_device", I, T_G_C, layout, camera, d_depth, depth_n_bytes, d_color,
                               color_n_bytes, counts, true);
}

int vgx_tsdf_projective_box(const vgx_depth_image_layout* layout, const vgx_depth_camera* camera, const vgx_tsdf_config* cfg,
                            const float T_G_C[7], float voxel_size, int32_t voxels_per_side, int32_t lo[3], int32_t hi[3]) {
  if (!cfg || !T_G_C || !lo || !hi) return VGX_ERR_INVALID;
  // (what the layout and the camera alone decide: the byte counts are not this call's business)
  const int rc = vgx_depth_image_check(layout, camera, INT64_MAX, INT64_MAX);
  if (rc != VGX_OK) return rc;
  return projective_box(*layout, *camera, *cfg, T_G_C, voxel_size, voxels_per_side, lo, hi, nullptr);
}

}  // extern "C"
