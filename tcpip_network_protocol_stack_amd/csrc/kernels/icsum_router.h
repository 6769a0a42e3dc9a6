// icsum_router.h — the router batch (k_router_ttl, k_router_hdrs) and its
// launchers.
#pragma once

#include "icsum_ipv4.h"
#include "icsum_route.h"

namespace icsum {
namespace {

// --------------------------------------------------- router batch -------
// Two lanes per datagram: lane 0 loads header dwords 0, 2, 4 and lane 1
// dwords 1, 3, 5, so each wave instruction touches 32 header lines with two
// neighbouring dwords each instead of 64 lines with one (one lane loading all
// six dwords: six instructions of 64 lines; the memory side then saw ~1.9
// 128-byte read requests per datagram for ~1.16 lines of header).  Measured
// (git 7692616:tools/probe/router_probe.hip, profiles/r2_router_probe.jsonl): 1 M x 1500 B
// 59.8 -> 57.3 us; the read-only floor of the same headers is 35-41 us, the
// rest is the scattered 8-byte write-back of every forwarded header.
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
    const bool valid = i < n;
    uint64_t s, e;
    seg_bounds(offsets, stride, dlen, valid ? i : n - 1, s, e, bsh);
    const bool hdr = valid && e - s >= 20;
    uint8_t* p = dg + s;
    const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
    // a datagram too short for a header (or an idle pair) reads the zero pad
    const uint32_t* q = hdr ? reinterpret_cast<const uint32_t*>(p - sh) : zpad;
    const uint32_t* last = hdr ? last_dword(dg + e) : zpad + 7;
    uint32_t mine[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t* a = q + (lane + 2u * k);
#ifdef ICSUM_BOUNDS_CHECK
      if (hdr && k < 2 && a > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(a));
#endif
      mine[k] = *(a < last ? a : last);
    }
    const int pair = int(threadIdx.x & 63u & ~1u);
    uint32_t d[6];
#pragma unroll
    for (int w = 0; w < 6; ++w) d[w] = uint32_t(__shfl(int(mine[w / 2]), pair + (w & 1), 64));
    if (valid && lane == 0) {
      uint8_t st = 0;
      [[maybe_unused]] uint32_t r_if = kNoRoute, r_hop = 0u;
      if (hdr) {
        Hdr h;
#pragma unroll
        for (int k = 0; k < 5; ++k) h.w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
        const uint32_t ver = h.byte(0) >> 4, hlen = h.byte(0) & 0x0fu, ttl = h.byte(8);
        // NetworkInterface::recv_frame parse (network_interface.cpp:51) then
        // Router::route: ttl <= 1 dropped, else ttl-- and compute_checksum()
        if (ver == 4 && hlen >= 5 && fold_value(ipv4_header_sum(h)) == h.be16(10) && ttl > 1) {
          h.w[2] = (h.w[2] & ~0xffu) | (ttl - 1);
          const uint32_t c = fold_value(ipv4_header_sum(h));
          if (sh == 0) {
            // dword-aligned header (every fixed stride that is a multiple of 4):
            // wire bytes 4..11 rewritten by ONE 8-byte store instead of three
            // narrow ones — id and fragment offset as read, the flags byte
            // re-serialized (reserved bit dropped), ttl - 1, protocol, checksum
            const uint32_t w1 = h.w[1] & ~0x00800000u;
            const uint32_t w2 = (h.w[2] & 0x0000ffffu) | ((c >> 8) << 16) | ((c & 0xffu) << 24);
            uint32_t* o = reinterpret_cast<uint32_t*>(p + 4);  // 4-byte aligned: merged to one dwordx2 store
            o[0] = w1;
            o[1] = w2;
          } else {
            p[6] = uint8_t(h.byte(6) & 0x7fu);  // re-serialized flags word
            p[8] = uint8_t(ttl - 1);
            store_be16(p + 10, c);
          }
          st = 1;
          if constexpr (kRoute) {
            if (route_find(rt, __builtin_bswap32(h.w[4]), r_if, r_hop)) st = 3;
          }
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

// Router batch with the forwarded headers apart.  Router::route decrements
// the ttl, recomputes the header checksum and hands send_datagram the
// datagram (router.cpp:39-66), which serialize() turns into two pieces: the
// 20 serialized header bytes (ipv4_header.cpp:62-86: options never written,
// the reserved flag bit dropped) and the payload after the parsed header
// (4 hlen bytes in, ipv4_header.cpp:50).  Here the payloads stay where they
// are (read-only batch) and the forwarded headers go to one coalesced array,
// 20 bytes per datagram: a forwarded datagram's header there is byte for
// byte what the in-place k_router_ttl leaves in its first 20 bytes; a
// dropped or unparseable one gets 20 zero bytes.  Headers are read as in
// k_router_ttl (two lanes per datagram, three dwords each); each wave stages
// its 32 headers in LDS and stores them as 160 consecutive dwords.
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
    uint64_t s, e;
    seg_bounds(offsets, stride, dlen, valid ? i : n - 1, s, e, bsh);
    const bool hdr = valid && e - s >= 20;
    const uint8_t* p = dg + s;
    const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
    const uint32_t* q = hdr ? reinterpret_cast<const uint32_t*>(p - sh) : zpad;
    const uint32_t* last = hdr ? last_dword(dg + e) : zpad + 7;
    uint32_t mine[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t* a = q + (lane + 2u * k);
#ifdef ICSUM_BOUNDS_CHECK
      if (hdr && k < 2 && a > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(a));
#endif
      mine[k] = *(a < last ? a : last);
    }
    const int pair = int(lane64 & ~1u);
    uint32_t d[6];
#pragma unroll
    for (int w = 0; w < 6; ++w) d[w] = uint32_t(__shfl(int(mine[w / 2]), pair + (w & 1), 64));
    Hdr h;
#pragma unroll
    for (int k = 0; k < 5; ++k) h.w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    const uint32_t ver = h.byte(0) >> 4, hlen = h.byte(0) & 0x0fu, ttl = h.byte(8);
    // NetworkInterface::recv_frame parse (network_interface.cpp:51), then
    // Router::route: ttl <= 1 dropped, else ttl-- and compute_checksum()
    const bool fwd = hdr && ver == 4 && hlen >= 5 && fold_value(ipv4_header_sum(h)) == h.be16(10) && ttl > 1;
    h.w[2] = (h.w[2] & ~0xffu) | ((ttl - 1) & 0xffu);
    const uint32_t c = fold_value(ipv4_header_sum(h));
    uint32_t o[5];
    o[0] = h.w[0];
    o[1] = h.w[1] & ~0x00800000u;  // the flags word re-serialized: reserved bit dropped
    o[2] = (h.w[2] & 0x0000ffffu) | ((c >> 8) << 16) | ((c & 0xffu) << 24);
    o[3] = h.w[3];
    o[4] = h.w[4];
    const uint32_t slot = (lane64 >> 1) * 5;
    for (uint32_t k = lane; k < 5; k += 2) sw[slot + k] = fwd ? o[k] : 0u;
    if constexpr (kRoute) {
      if (valid && lane == 0) {
        uint32_t r_if = kNoRoute, r_hop = 0u;
        const bool routed = fwd && route_find(rt, __builtin_bswap32(h.w[4]), r_if, r_hop);
        status[i] = fwd ? (routed ? 3 : 1) : 0;
        if (rt_iface) rt_iface[i] = r_if;
        if (rt_hop) rt_hop[i] = r_hop;
      }
    } else {
      if (valid && lane == 0) status[i] = fwd ? 1 : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the wave's datagrams [wbase, wbase + 32): 160 consecutive dwords of the array
    const uint64_t wbase = g0 + (threadIdx.x >> 6) * kPerWave;
    const uint64_t cnt = wbase < n ? (n - wbase < kPerWave ? n - wbase : kPerWave) : 0;
#pragma unroll
    for (uint32_t j = 0; j < 3; ++j) {
      const uint32_t t = j * 64u + lane64;
      if (t < cnt * 5) hdr_out[wbase * 5 + t] = sw[t];
    }
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
