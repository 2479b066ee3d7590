// The chain clock (voxgraph_amd/csrc/vgx_chain_clock.h) in a program of its own, built with AddressSanitizer and UBSan by
// tests/test_chain_clock_cpu.py.  It includes nothing else of the library.  It runs named sequences of takes from stated
// starting clocks and prints every take; the test recomputes every line from the stated rule.
//
//   S <name> <epoch> <tickets>                               a sequence starts from this clock
//   T <tiles> <epoch> <ticket_base> <clear_first: 0 | 1> <clock epoch after> <clock tickets after>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "vgx_chain_clock.h"

namespace {

vgx::ChainClock begin(const char* name, uint32_t epoch, uint32_t tickets) {
  vgx::ChainClock c;
  c.epoch = epoch;
  c.tickets = tickets;
  std::printf("S %s %u %u\n", name, (unsigned)epoch, (unsigned)tickets);
  return c;
}

void take(vgx::ChainClock& c, uint32_t tiles) {
  const vgx::ChainTake t = c.take(tiles);
  std::printf("T %u %u %u %d %u %u\n", (unsigned)tiles, (unsigned)t.epoch, (unsigned)t.ticket_base, t.clear_first ? 1 : 0,
              (unsigned)c.epoch, (unsigned)c.tickets);
}

uint64_t state = 0x2545f4914f6cdd1dull;
uint32_t draw() {  // splitmix64, the top 32 bits
  state += 0x9e3779b97f4a7c15ull;
  uint64_t z = state;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (uint32_t)(z >> 32);
}

}  // namespace

int main() {
  const uint32_t max = (uint32_t)vgx::kChainEpochMax;
  {  // a new handle (a default-constructed clock): epochs 1, 2, 3, ...; the tile counts the kernels meet and the largest
    vgx::ChainClock c;
    std::printf("S fresh %u %u\n", (unsigned)c.epoch, (unsigned)c.tickets);
    for (uint32_t tiles : {1u, 64u, 65u, 1u << 24, 1u << 31, 1u << 31, 68u, 0u, 75u}) take(c, tiles);
    for (int i = 0; i < 200; ++i) take(c, 68u);
  }
  {  // the rollover: Max - 1 -> Max, no clear -> clear and 1 -> 2 ...
    vgx::ChainClock c = begin("rollover", max - 1, 136u);
    for (int i = 0; i < 6; ++i) take(c, 68u);
  }
  {  // ... and a second one right behind it (a clock set to Max itself), launches that take no tickets among them
    vgx::ChainClock c = begin("at_max", max, 7u);
    for (uint32_t tiles : {0u, 0u, 5u, 0u}) take(c, tiles);
    c.epoch = max - 2;
    std::printf("S again %u %u\n", (unsigned)c.epoch, (unsigned)c.tickets);
    for (uint32_t tiles : {3u, 0u, 0u, 9u, 1u}) take(c, tiles);
  }
  {  // a take that straddles 2^32, one that ends exactly on it, and one that starts there
    vgx::ChainClock c = begin("straddle", 41u, 0xffffffffu - 29u);
    take(c, 68u);
    take(c, 68u);
    c = begin("exact", 41u, 0xffffffffu - 67u);
    take(c, 68u);
    take(c, 68u);
    c = begin("halves", 0u, 1u << 31);
    take(c, 1u << 31);
    take(c, 1u << 31);
    take(c, 0xffffffffu);
    take(c, 0xffffffffu);
  }
  for (int s = 0; s < 16; ++s) {  // seeded: starts a few launches before the rollover, tickets anywhere, tile counts of every size
    vgx::ChainClock c = begin("seeded", max - draw() % 12u, draw());
    for (int i = 0; i < 24; ++i) {
      const uint32_t r = draw();
      const uint32_t tiles = i % 5 == 0 ? 0u : (i % 5 == 1 ? r : (i % 5 == 2 ? r >> 8 : (r >> 20) + 1u));
      take(c, tiles);
    }
  }
  std::printf("chain_clock_check ok\n");
  return 0;
}
