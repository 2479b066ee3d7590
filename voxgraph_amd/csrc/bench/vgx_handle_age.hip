// Handle age for the tests (include/voxgraph_amd_bench.h; libvoxgraph_amd_bench.so): reads and sets the chain clocks
// (ChainClock, csrc/vgx_chain_clock.h) of a decoded scan and of a TSDF integrator, so that tests/test_handle_age_gpu.py can
// put a handle a few launches before an epoch rollover or a ticket wrap that real use reaches after days or weeks.  The
// setters change what the host will hand the next launch, and the device ticket word with it; they never touch the tile
// words -- the stale tags real launches left there are what the rollover has to cope with.
#include "vgx_projective_kernel.h"
#include "vgx_tsdf_internal.h"
#include "voxgraph_amd_bench.h"

using namespace vgx;

namespace {

bool epoch_in_range(int64_t epoch) { return epoch >= 0 && epoch <= (int64_t)kChainEpochMax; }
bool tickets_in_range(int64_t tickets) { return tickets >= 0 && tickets <= (int64_t)UINT32_MAX; }

// tickets, zero-extended, into the device's ticket word behind everything queued on the TSDF stream (the caller holds
// ctx->tsdf_mu); waits for it
int write_ticket_word(vgx_ctx ctx, unsigned long long* d_word, uint32_t tickets) {
  const unsigned long long word = tickets;
  VGX_HIP(ctx, hipSetDevice(ctx->device));
  VGX_HIP(ctx, hipMemcpyAsync(d_word, &word, 8, hipMemcpyHostToDevice, ctx->tsdf_stream));
  VGX_HIP(ctx, hipStreamSynchronize(ctx->tsdf_stream));
  return VGX_OK;
}

}  // namespace

extern "C" {

int vgx_scan_set_age(vgx_scan S, int64_t epoch, int64_t tickets) {
  if (!S) return VGX_ERR_INVALID;
  vgx_ctx ctx = S->ctx;
  if (!epoch_in_range(epoch)) return set_error(ctx, VGX_ERR_INVALID, "vgx_scan_set_age: epoch is not in 0 .. 2^30 - 1");
  if (!tickets_in_range(tickets)) return set_error(ctx, VGX_ERR_INVALID, "vgx_scan_set_age: tickets is not in 0 .. 2^32 - 1");
  std::lock_guard<std::mutex> lk(S->mu);  // (the locks of a decode, in its order)
  std::lock_guard<std::mutex> tsdf_lk(ctx->tsdf_mu);
  if (!S->d_ctl.p) return set_error(ctx, VGX_ERR_INVALID, "vgx_scan_set_age: the scan has not decoded anything yet");
  const int rc = write_ticket_word(ctx, S->d_ctl.as<unsigned long long>() + kScanTicket, (uint32_t)tickets);
  if (rc != VGX_OK) return rc;
  S->clock.epoch = (uint32_t)epoch;
  S->clock.tickets = (uint32_t)tickets;
  return VGX_OK;
}

int vgx_scan_get_age(vgx_scan S, int64_t* epoch, int64_t* tickets) {
  if (!S) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(S->mu);
  if (epoch) *epoch = (int64_t)S->clock.epoch;
  if (tickets) *tickets = (int64_t)S->clock.tickets;
  return VGX_OK;
}

int vgx_tsdf_integrator_set_projective_age(vgx_tsdf_integrator I, int64_t epoch, int64_t tickets) {
  if (!I) return VGX_ERR_INVALID;
  vgx_ctx ctx = I->ctx;
  if (!epoch_in_range(epoch))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_tsdf_integrator_set_projective_age: epoch is not in 0 .. 2^30 - 1");
  if (!tickets_in_range(tickets))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_tsdf_integrator_set_projective_age: tickets is not in 0 .. 2^32 - 1");
  std::lock_guard<std::mutex> own(I->mu);  // (the locks of a frame, in its order)
  std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
  if (!I->d_proj_ctl.p)
    return set_error(ctx, VGX_ERR_INVALID, "vgx_tsdf_integrator_set_projective_age: no frame has been integrated yet");
  const int rc = write_ticket_word(ctx, I->d_proj_ctl.as<unsigned long long>() + kProjTicket, (uint32_t)tickets);
  if (rc != VGX_OK) return rc;
  I->proj_clock.epoch = (uint32_t)epoch;
  I->proj_clock.tickets = (uint32_t)tickets;
  return VGX_OK;
}

int vgx_tsdf_integrator_get_projective_age(vgx_tsdf_integrator I, int64_t* epoch, int64_t* tickets) {
  if (!I) return VGX_ERR_INVALID;
  std::lock_guard<std::mutex> own(I->mu);
  if (epoch) *epoch = (int64_t)I->proj_clock.epoch;
  if (tickets) *tickets = (int64_t)I->proj_clock.tickets;
  return VGX_OK;
}

int vgx_tsdf_integrator_set_reproducible_age(vgx_tsdf_integrator I, int64_t epoch) {
  if (!I) return VGX_ERR_INVALID;
  vgx_ctx ctx = I->ctx;
  if (!epoch_in_range(epoch))
    return set_error(ctx, VGX_ERR_INVALID, "vgx_tsdf_integrator_set_reproducible_age: epoch is not in 0 .. 2^30 - 1");
  std::lock_guard<std::mutex> own(I->mu);  // (the locks of a scan, in its order)
  std::lock_guard<std::mutex> lk(ctx->tsdf_mu);
  if (!I->det)
    return set_error(ctx, VGX_ERR_INVALID,
                     "vgx_tsdf_integrator_set_reproducible_age: no reproducible or merged scan has been integrated yet");
  I->det_clock.epoch = (uint32_t)epoch;  // (the tickets restart with every scan)
  return VGX_OK;
}

int vgx_tsdf_integrator_get_reproducible_age(vgx_tsdf_integrator I, int64_t* epoch) {
  if (!I) return VGX_ERR_INVALID;
  vgx_ctx ctx = I->ctx;
  std::lock_guard<std::mutex> own(I->mu);
  if (!I->det)
    return set_error(ctx, VGX_ERR_INVALID,
                     "vgx_tsdf_integrator_get_reproducible_age: no reproducible or merged scan has been integrated yet");
  if (epoch) *epoch = (int64_t)I->det_clock.epoch;
  return VGX_OK;
}

}  // extern "C"
