// icsum_neigh.h — internal to libicsum.so: the compiled image of a neighbour
// table (icsum_neigh.cpp) as the device path (icsum_images.cpp) takes it.
// Plain C++, no HIP.  Not installed, not part of the ABI.
//
// Image: one uint32 array, 4 * nif identity words, then 4 * nslots slot words.
//   identity  entry f (interface f, 0 <= f < nif), 16 bytes:
//             [0] mac bytes 0..3 as they lie in memory
//             [1] mac bytes 4..5 | kNeighConfigured when set_iface gave the addresses
//             [2] the interface's IPv4 address, host order
//             [3] 0
//   slot      16 bytes, nslots a power of two >= max(4, 2 * mappings):
//             [0] ip, host order
//             [1] iface | kNeighUsed   (0: an empty slot)
//             [2] mac bytes 0..3
//             [3] mac bytes 4..5
// A key (iface, ip) lives at the first free slot from neigh_hash(iface, ip) &
// (nslots - 1), stepping by one and wrapping at the end of the array.  The load
// factor is at most 1/2, so every probe sequence ends at an empty slot; a probe
// is one aligned 16-byte load.  The image holds no timers: ageing changes it
// only when a mapping is erased.
#pragma once

#include <cstdint>

#include "icsum.h"

namespace icsum::detail {

constexpr uint32_t kNeighConfigured = 0x10000u;  // identity word 1
constexpr uint32_t kNeighUsed = 0x80000000u;     // slot word 1
constexpr uint32_t kNeighMaxIface = 65536;

struct NeighImageView {
  uint64_t id = 0;   // the table's id, unique in this library for the process's life
  uint64_t gen = 0;  // changes when the image's contents change
  const uint32_t* words = nullptr;  // 4 * nif + 4 * nslots words
  uint32_t nif = 0, nslots = 0;
};

// Compile the table if it changed and lock it: `view` stays valid until
// neigh_image_release.  ICS_OK or an error code (message set).
int neigh_image_acquire(ics_neigh_table* tbl, NeighImageView* view);
void neigh_image_release(ics_neigh_table* tbl);

// lowbias32 over the key; the device (kernels/icsum_frame.h) and the tests'
// restatement compute the same.
inline uint32_t neigh_hash(uint32_t iface, uint32_t ip) {
  uint32_t h = ip ^ (iface * 0x9E3779B1u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// One lookup in an image's slots (`slots` = words + 4 * nif); the device walks
// the same words.  The slot, or null on a miss.
inline const uint32_t* neigh_walk(const uint32_t* slots, uint32_t nslots, uint32_t iface, uint32_t ip) {
  const uint32_t mask = nslots - 1, key = iface | kNeighUsed;
  uint32_t at = neigh_hash(iface, ip) & mask;
  for (uint32_t probes = 0; probes < nslots; ++probes, at = (at + 1) & mask) {
    const uint32_t* s = slots + 4 * uint64_t(at);
    if (s[1] == 0u) return nullptr;
    if (s[0] == ip && s[1] == key) return s;
  }
  return nullptr;
}

}  // namespace icsum::detail
