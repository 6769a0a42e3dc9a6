// icsum_route.h — Router::match on the device: the trie walk the router
// kernels fuse (icsum_router.h), the lookup-only batch (k_route_lookup) and
// its launcher.  The image is the one icsum_route.cpp compiles and walks on
// the host (csrc/icsum_route.h): 1 to 3 dependent word loads, then one 8-byte
// record load.  A table without routes longer than /16 is 256 KiB.
#pragma once

#include "icsum_common.h"

namespace icsum {
namespace {

constexpr uint32_t kRouteChild = 0x80000000u, kRouteDirect = 0x80000000u, kNoRoute = 0xFFFFFFFFu;

// one trie word; the bounds-checked build reports an index outside the image
// and reads nothing (the walk then ends on "no route")
__device__ __forceinline__ uint32_t route_word(const RouteImg& t, uint64_t at) {
#ifdef ICSUM_BOUNDS_CHECK
  if (at >= t.nwords) {
    bounds_fail(kBoundsRoute, at);
    return 0u;
  }
#endif
  return t.words[at];
}

// match(addr): false = no route (iface = 0xFFFFFFFF, next_hop = 0)
__device__ __forceinline__ bool route_find(const RouteImg& t, uint32_t addr, uint32_t& iface, uint32_t& next_hop) {
  uint32_t x = route_word(t, addr >> 16);
  if (x & kRouteChild) {
    x = route_word(t, uint64_t(x & ~kRouteChild) + ((addr >> 8) & 255u));
    if (x & kRouteChild) x = route_word(t, uint64_t(x & ~kRouteChild) + ((addr >> 1) & 127u));
  }
  iface = kNoRoute;
  next_hop = 0u;
#ifdef ICSUM_BOUNDS_CHECK
  if (x && x - 1u >= t.nrecs) {
    bounds_fail(kBoundsRoute, t.nwords + 2ull * (x - 1u));
    return false;
  }
#endif
  if (x == 0u) return false;
  // nwords is even and the image 8-byte aligned: one dwordx2 load
  const uint2 r = *reinterpret_cast<const uint2*>(t.words + t.nwords + 2ull * (x - 1u));
  iface = r.x & ~kRouteDirect;
  next_hop = (r.x & kRouteDirect) ? addr : r.y;  // next_hop.value_or(dst)
  return true;
}

// One lane per host-order address; both outputs coalesced.
__global__ __launch_bounds__(kBlock) void k_route_lookup(const uint32_t* __restrict__ addrs, uint64_t n, RouteImg t,
                                                         uint32_t* __restrict__ iface,
                                                         uint32_t* __restrict__ next_hop) {
  const uint64_t step = uint64_t(gridDim.x) * kBlock;
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n; i += step) {
    uint32_t f, h;
    route_find(t, addrs[i], f, h);
    if (iface) iface[i] = f;
    if (next_hop) next_hop[i] = h;
  }
}

}  // namespace

hipError_t launch_route_lookup(const uint32_t* addrs, uint64_t n, const RouteImg& t, uint32_t* iface,
                               uint32_t* next_hop, hipStream_t st) {
  hipLaunchKernelGGL(k_route_lookup, dim3(ew_blocks(n)), dim3(kBlock), 0, st, addrs, n, t, iface, next_hop);
  return hipGetLastError();
}

}  // namespace icsum
