// The host bookkeeping of a TileChain launch (vgx_tsdf_internal.h), in one place and in plain C++: this header has no HIP
// in it, so tests/cpp/chain_clock_check.cpp builds it alone, and the tooling library reads and sets the clocks of
// long-lived handles through it (include/voxgraph_amd_bench.h, "handle age").
//
// A chain's tile words are tagged with the launch's epoch, 1 .. kChainEpochMax (30 bits of the 64-bit word: epoch << 34 |
// status << 32 | value), so that no word is cleared between launches; the tiles of a launch are the tickets taken from one
// device word that only counts up, minus what the host has launched on it before (`ticket_base`, modulo 2^32 like the
// device's subtraction).  After kChainEpochMax launches the tags start over at 1, and the words -- whose stale tags could
// otherwise be met again -- are cleared first.
#ifndef VGX_CHAIN_CLOCK_H_
#define VGX_CHAIN_CLOCK_H_

#include <cstdint>

namespace vgx {

constexpr unsigned long long kChainEpochMax = (1ull << 30) - 1;

struct ChainTake {
  uint32_t epoch;        // 1 .. kChainEpochMax: the launch's tag
  uint32_t ticket_base;  // the tickets launched on the device word before this launch, mod 2^32
  bool clear_first;      // the tags have started over: the caller zeroes the tile words on the stream ahead of the launch
};

struct ChainClock {
  uint32_t epoch = 0;    // the last launch's tag (0: none yet, or the words have just been zeroed)
  uint32_t tickets = 0;  // what the device's ticket word reads once everything launched has started, mod 2^32

  // The next launch, over `tiles` workgroups.  (tiles == 0: a launch that shares the words and the epochs but takes its
  // tiles from another counter -- the reproducible mode's sweeps.)
  ChainTake take(uint32_t tiles) {
    ChainTake t;
    t.clear_first = epoch >= kChainEpochMax;
    if (t.clear_first) epoch = 0;
    t.epoch = ++epoch;
    t.ticket_base = tickets;
    tickets += tiles;
    return t;
  }
};

}  // namespace vgx

#endif  // VGX_CHAIN_CLOCK_H_
