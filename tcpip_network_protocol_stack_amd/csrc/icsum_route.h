// icsum_route.h — internal to libicsum.so: the compiled image of a route
// table (icsum_route.cpp) as the device path (icsum_images.cpp) takes it.
// Plain C++, no HIP.  Not installed, not part of the ABI.
//
// Image: nwords trie words, then two words per route record.
//   level 1  65536 words indexed by addr >> 16
//   level 2  chunks of 256 words indexed by (addr >> 8) & 255
//   level 3  chunks of 128 words indexed by (addr >> 1) & 127  (bit 0 never matches)
//   word     bit 31 set: child chunk at word index (word & 0x7fffffff)
//            else a leaf: 0 = no route, k + 1 = route record k
//   record   iface | (direct ? 0x80000000 : 0), next_hop
#pragma once

#include <cstdint>

#include "icsum.h"

namespace icsum::detail {

constexpr uint32_t kRouteChild = 0x80000000u;   // trie word: child pointer
constexpr uint32_t kRouteDirect = 0x80000000u;  // record word 0: no next hop, the answer is dst itself
constexpr uint64_t kRouteL1Words = 65536, kRouteL2Words = 256, kRouteL3Words = 128;

struct RouteImageView {
  uint64_t id = 0;   // the table's id, unique in this library for the process's life
  uint64_t gen = 0;  // changes with every add / clear
  const uint32_t* words = nullptr;  // nwords + 2 * nrecs words
  uint64_t nwords = 0;
  uint32_t nrecs = 0;
};

// Compile the table if it changed and lock it: `view` stays valid until
// route_image_release.  ICS_OK or an error code (message set).
int route_image_acquire(ics_route_table* tbl, RouteImageView* view);
void route_image_release(ics_route_table* tbl);

// One lookup in an image; the device kernels (kernels/icsum_route.h) walk the
// same words.  Returns the leaf (0: no route).
inline uint32_t route_walk(const uint32_t* w, uint32_t addr) {
  uint32_t x = w[addr >> 16];
  if (x & kRouteChild) {
    x = w[uint64_t(x & ~kRouteChild) + ((addr >> 8) & 255u)];
    if (x & kRouteChild) x = w[uint64_t(x & ~kRouteChild) + ((addr >> 1) & 127u)];
  }
  return x;
}

}  // namespace icsum::detail
