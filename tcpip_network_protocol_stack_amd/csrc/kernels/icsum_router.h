// icsum_router.h — the router batch (k_router_ttl, k_router_hdrs) and its
// launchers.
#pragma once

#include "icsum_hdrpass.h"
#include "icsum_route.h"

namespace icsum {
namespace {

// --------------------------------------------------- router batch -------
// Two lanes per datagram (pair_hdr_load); lane 0 of the pair decides and
// rewrites in place (hdr_parses, hop_rewrite).
// kRoute: Router::route's second half fused (router.cpp:53-66): a datagram
// that forwards looks its dst (already in registers) up in the route image —
// after the rewrite, as the reference matches after compute_checksum() —
// status gains bit 1 on a match, and iface / next_hop (nullable) receive the
// answer or the no-route values.  <false> is the bare step, unchanged.
template <bool kRoute>
__global__ __launch_bounds__(kBlock) void k_router_ttl(uint8_t* __restrict__ dg,
                                                       const uint64_t* __restrict__ offsets,
                                                       uint64_t stride, uint64_t dlen, uint64_t n,
                                                       uint8_t* __restrict__ status,
                                                       const uint32_t* __restrict__ zpad, RouteImg rt,
                                                       uint32_t* __restrict__ rt_iface,
                                                       uint32_t* __restrict__ rt_hop) {
  constexpr uint32_t kG = kBlock / 2;
  const uint32_t lane = threadIdx.x & 1u;
  const uint64_t step = uint64_t(gridDim.x) * kG;
  const uint32_t bsh = frame_shift(dg);
  dg -= bsh;
  // the loop bound is uniform per block (group base index), so both lanes of
  // every pair reach the shuffles together
  for (uint64_t g0 = uint64_t(blockIdx.x) * kG; g0 < n; g0 += step) {
    const uint64_t i = g0 + threadIdx.x / 2;
    Hdr h;
    uint32_t sh;
    uint64_t s;
    const bool hdr = pair_hdr_load(dg, offsets, stride, dlen, n, bsh, i, zpad, h, sh, s);
    if (i < n && lane == 0) {
      uint8_t st = 0;
      [[maybe_unused]] uint32_t r_if = kNoRoute, r_hop = 0u;
      // Router::route: ttl <= 1 dropped
      if (hdr && hdr_parses(h) && h.byte(8) > 1) {
        uint32_t o[5];
        hop_rewrite(h, o);
        uint8_t* p = dg + s;
        if (sh == 0) {
          // dword-aligned header (every fixed stride that is a multiple of 4):
          // wire bytes 4..11 rewritten by ONE 8-byte store instead of three
          // narrow ones — id and fragment offset as read, the flags byte
          // re-serialized, ttl - 1, protocol, checksum
          uint32_t* w = reinterpret_cast<uint32_t*>(p + 4);  // 4-byte aligned: merged to one dwordx2 store
          w[0] = o[1];
          w[1] = o[2];
        } else {
          p[6] = uint8_t(o[1] >> 16);  // re-serialized flags byte
          p[8] = uint8_t(o[2]);        // ttl - 1
          store_be16(p + 10, bswap32(o[2]) & 0xffffu);
        }
        st = 1;
        if constexpr (kRoute) {
          if (route_find(rt, bswap32(o[4]), r_if, r_hop)) st = 3;
        }
      }
      status[i] = st;
      if constexpr (kRoute) {
        if (rt_iface) rt_iface[i] = r_if;
        if (rt_hop) rt_hop[i] = r_hop;
      }
    }
  }
}

// Router batch with the forwarded headers apart.  Router::route hands
// send_datagram the rewritten datagram, which serialize() turns into two
// pieces: the 20 serialized header bytes (hop_rewrite) and the payload after
// the parsed header (4 hlen bytes in, ipv4_header.cpp:50).  Here the payloads
// stay where they are (read-only batch) and the forwarded headers go to one
// coalesced array, 20 bytes per datagram: a forwarded datagram's header there
// is byte for byte what the in-place k_router_ttl leaves in its first 20
// bytes; a dropped or unparseable one gets 20 zero bytes.  Headers are read
// as in k_router_ttl; each wave stages its 32 headers in LDS and stores them
// as 160 consecutive dwords (wave_store).
// kRoute: as k_router_ttl<true>; lane 0 of a forwarding pair walks the trie.
template <bool kRoute>
__global__ __launch_bounds__(kBlock) void k_router_hdrs(const uint8_t* __restrict__ dg,
                                                        const uint64_t* __restrict__ offsets, uint64_t stride,
                                                        uint64_t dlen, uint64_t n, uint32_t* __restrict__ hdr_out,
                                                        uint8_t* __restrict__ status,
                                                        const uint32_t* __restrict__ zpad, RouteImg rt,
                                                        uint32_t* __restrict__ rt_iface,
                                                        uint32_t* __restrict__ rt_hop) {
  constexpr uint32_t kG = kBlock / 2, kPerWave = 32;
  __shared__ uint32_t stage[kBlock / 64][kPerWave * 5];
  const uint32_t lane = threadIdx.x & 1u, lane64 = threadIdx.x & 63u;
  uint32_t* const sw = stage[threadIdx.x >> 6];
  const uint64_t step = uint64_t(gridDim.x) * kG;
  const uint32_t bsh = frame_shift(dg);
  dg -= bsh;
  for (uint64_t g0 = uint64_t(blockIdx.x) * kG; g0 < n; g0 += step) {  // uniform per block
    const uint64_t i = g0 + threadIdx.x / 2;
    const bool valid = i < n;
    Hdr h;
    uint32_t sh;
    uint64_t s;
    const bool hdr = pair_hdr_load(dg, offsets, stride, dlen, n, bsh, i, zpad, h, sh, s);
    // Router::route: ttl <= 1 dropped
    const bool fwd = hdr && hdr_parses(h) && h.byte(8) > 1;
    uint32_t o[5];
    hop_rewrite(h, o);
    const uint32_t slot = (lane64 >> 1) * 5;
    for (uint32_t k = lane; k < 5; k += 2) sw[slot + k] = fwd ? o[k] : 0u;
    if constexpr (kRoute) {
      if (valid && lane == 0) {
        uint32_t r_if = kNoRoute, r_hop = 0u;
        const bool routed = fwd && route_find(rt, bswap32(o[4]), r_if, r_hop);
        status[i] = fwd ? (routed ? 3 : 1) : 0;
        if (rt_iface) rt_iface[i] = r_if;
        if (rt_hop) rt_hop[i] = r_hop;
      }
    } else {
      if (valid && lane == 0) status[i] = fwd ? 1 : 0;
    }
    // the wave's datagrams [wbase, wbase + 32)
    wave_store<5, kPerWave>(sw, hdr_out, g0 + (threadIdx.x >> 6) * kPerWave, n, lane64);
    __builtin_amdgcn_wave_barrier();  // the next pass rewrites sw
  }
}

}  // namespace

hipError_t launch_router_hdrs(const SegSpec& sp, uint32_t* hdr_out, uint8_t* status, hipStream_t st) {
  hipLaunchKernelGGL(k_router_hdrs<false>, dim3(ew_blocks(sp.n * 2)), dim3(kBlock), 0, st, sp.bytes, sp.offsets,
                     sp.stride, sp.seg_len, sp.n, hdr_out, status, static_cast<const uint32_t*>(sp.zero16),
                     RouteImg{}, nullptr, nullptr);
  return hipGetLastError();
}

hipError_t launch_router_ttl(const SegSpec& sp, uint8_t* status, hipStream_t st) {
  hipLaunchKernelGGL(k_router_ttl<false>, dim3(ew_blocks(sp.n * 2)), dim3(kBlock), 0, st,
                     const_cast<uint8_t*>(sp.bytes), sp.offsets, sp.stride, sp.seg_len, sp.n, status,
                     static_cast<const uint32_t*>(sp.zero16), RouteImg{}, nullptr, nullptr);
  return hipGetLastError();
}

hipError_t launch_router_route(const SegSpec& sp, const RouteImg& t, uint32_t* hdr_out, uint8_t* status,
                               uint32_t* iface, uint32_t* next_hop, hipStream_t st) {
  const uint32_t* zpad = static_cast<const uint32_t*>(sp.zero16);
  if (hdr_out)
    hipLaunchKernelGGL(k_router_hdrs<true>, dim3(ew_blocks(sp.n * 2)), dim3(kBlock), 0, st, sp.bytes, sp.offsets,
                       sp.stride, sp.seg_len, sp.n, hdr_out, status, zpad, t, iface, next_hop);
  else
    hipLaunchKernelGGL(k_router_ttl<true>, dim3(ew_blocks(sp.n * 2)), dim3(kBlock), 0, st,
                       const_cast<uint8_t*>(sp.bytes), sp.offsets, sp.stride, sp.seg_len, sp.n, status, zpad, t,
                       iface, next_hop);
  return hipGetLastError();
}

}  // namespace icsum
