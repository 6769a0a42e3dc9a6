// icsum_frame.h — Ethernet frames through the router hop (k_frame) and its
// launcher: NetworkInterface::recv_frame's data-plane half
// (network_interface.cpp:40-87: destination filter, type branch, IPv4 / ARP
// parse) and, fused behind it, Router::route (router.cpp:27-70) up to
// send_datagram's cache lookup and make_frame's header
// (network_interface.cpp:18-37, :115-118).  The control half — learning,
// timers, requests and replies — is the host table of icsum_neigh.cpp, whose
// compiled image (csrc/icsum_neigh.h) the kernel reads.
#pragma once

#include "icsum_hdrpass.h"
#include "icsum_route.h"

namespace icsum {
namespace {

constexpr uint32_t kNeighConfigured = 0x10000u, kNeighUsed = 0x80000000u;
constexpr uint32_t kFrResolved = 0x04u, kFrDgram = 0x08u, kFrForUs = 0x10u, kFrIpv4 = 0x20u, kFrArp = 0x40u,
                   kFrArpOk = 0x80u;

// icsum_neigh.h's neigh_hash
__device__ __forceinline__ uint32_t neigh_hash(uint32_t iface, uint32_t ip) {
  uint32_t h = ip ^ (iface * 0x9E3779B1u);
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

// interface f's identity entry (mac 0..3, mac 4..5 | configured, ip, 0); an
// interface beyond the array was never configured: zeros, nothing read
__device__ __forceinline__ u32x4 neigh_ident(const NeighImg& t, uint32_t f) {
  const u32x4 none = {0u, 0u, 0u, 0u};
  if (f >= t.nif) return none;
  return *reinterpret_cast<const u32x4*>(t.words + 4ull * f);
}

// arp_addr_table_.find(ip) on interface f: linear probing from the hash,
// wrapping, one 16-byte load per probe, ended by an empty slot (the builder
// keeps the load factor <= 1/2).  The probe count is bounded by the slot
// count, so a damaged image cannot hold a lane; the bounds-checked build
// reports it, and any slot index outside the table.
__device__ __forceinline__ bool neigh_find(const NeighImg& t, uint32_t f, uint32_t ip, uint32_t& m_lo,
                                           uint32_t& m_hi) {
  const u32x4* __restrict__ slots = reinterpret_cast<const u32x4*>(t.words + 4ull * t.nif);
  const uint32_t mask = t.nslots - 1u, key = f | kNeighUsed;
  uint32_t at = neigh_hash(f, ip) & mask;
  for (uint32_t probes = 0; probes < t.nslots; ++probes, at = (at + 1u) & mask) {
#ifdef ICSUM_BOUNDS_CHECK
    if (at >= t.nslots) {
      bounds_fail(kBoundsNeigh, at);
      return false;
    }
#endif
    const u32x4 s = slots[at];
    if (s.y == 0u) return false;
    if (s.x == ip && s.y == key) {
      m_lo = s.z;
      m_hi = s.w;
      return true;
    }
  }
#ifdef ICSUM_BOUNDS_CHECK
  bounds_fail(kBoundsNeigh, at);  // no empty slot in the whole table
#endif
  return false;
}

// A header-only pass in rows (rows_load / row_take, icsum_hdrpass.h): a wave
// takes 64 consecutive frames per pass.  A frame's first 34 bytes are 14 of
// Ethernet, then the IPv4 header or the first 8 bytes of ARP; the parsing
// lane takes the header 14 bytes in by a fixed alignbyte of 2.  Every lane
// then works on a frame of its own: the route walk and the neighbour probe
// are gathers of 64 lanes, and status / iface / next hop are coalesced stores.
// (Shapes tried, 1 M x 1514 B, classification / whole hop: k_router_hdrs' two
// lanes per frame with five dword loads each 59.1 / 86.1 us; four lanes per
// frame with the dwordx4 load and the lookups on one lane in four 50.5 / 89.0
// us; this one: DESIGN.md §12.)
// kHop = false: d_status only (recv_frame's classification); the route image
// and the slots are not read.
// kHop = true: the forward decision and header rewrite of k_router_hdrs<true>
// on the datagram at frame + 14, the lookups, and one 36-byte record per frame
// — 2 zero bytes, the Ethernet header, the 20 forwarded header bytes — staged
// in LDS per wave (64 records, 576 dwords) and stored as consecutive dwords.
template <bool kHop>
__global__ __launch_bounds__(kBlock) void k_frame(const uint8_t* __restrict__ fr,
                                                  const uint64_t* __restrict__ offsets, uint64_t stride,
                                                  uint64_t flen, uint64_t n, uint32_t in_iface,
                                                  const uint32_t* __restrict__ in_ifaces,
                                                  uint32_t* __restrict__ hdr_out, uint8_t* __restrict__ status,
                                                  const uint32_t* __restrict__ zpad, RouteImg rt, NeighImg nb,
                                                  uint32_t* __restrict__ rt_iface, uint32_t* __restrict__ rt_hop) {
  constexpr uint32_t kRec = 9;
  __shared__ uint32_t raw[kBlock / 64][kRowsPerWave * kRow];
  __shared__ uint32_t stage[kHop ? kBlock / 64 : 1][kHop ? kRowsPerWave * kRec : 1];
  const uint32_t lane64 = threadIdx.x & 63u;
  uint32_t* const rw = raw[threadIdx.x >> 6];
  [[maybe_unused]] uint32_t* const sw = stage[kHop ? threadIdx.x >> 6 : 0];
  const uint64_t step = uint64_t(gridDim.x) * kBlock;
  const uint32_t bsh = frame_shift(fr);
  fr -= bsh;
  for (uint64_t g0 = uint64_t(blockIdx.x) * kBlock; g0 < n; g0 += step) {  // uniform per block
    const uint64_t wbase = g0 + (threadIdx.x >> 6) * kRowsPerWave;
    rows_load<14>(fr, offsets, stride, flen, n, bsh, wbase, lane64, zpad, rw);
    // ---- parse: lane l has frame wbase + l
    const uint64_t i = wbase + lane64;
    const bool valid = i < n;
    uint64_t s, e;
    seg_bounds(offsets, stride, flen, valid ? i : n - 1, s, e, bsh);
    const uint64_t len = item_len(s, e);
    const bool eth = valid && len >= 14;
    uint32_t f[9];
    row_take(rw, lane64, eth, s, f);
    Hdr h;  // frame bytes 14 .. 33: the IPv4 header, or ARP's fixed fields in w[0], w[1]
#pragma unroll
    for (int k = 0; k < 5; ++k) h.w[k] = __builtin_amdgcn_alignbyte(f[k + 4], f[k + 3], 2u);

    // recv_frame: dst is broadcast or the ingress interface's address
    const uint32_t fin = in_ifaces ? in_ifaces[valid ? i : n - 1] : in_iface;
    const u32x4 me = neigh_ident(nb, fin);
    const uint32_t dst_hi = f[1] & 0xffffu;
    const bool for_us = eth && (me.y & kNeighConfigured) &&
                        ((f[0] == 0xffffffffu && dst_hi == 0xffffu) || (f[0] == me.x && dst_hi == (me.y & 0xffffu)));
    const uint32_t type = f[3] & 0xffffu;  // bytes 12, 13 as they lie: 08 00 -> 0x0008, 08 06 -> 0x0608
    const bool ipv4 = for_us && type == 0x0008u, arp = for_us && type == 0x0608u;
    // ARPMessage::parse: 28 bytes and supported() — 00 01 08 00 | 06 04 00 op, op 1 or 2
    const bool arp_ok = arp && len >= 42 && h.w[0] == 0x00080100u &&
                        (h.w[1] == 0x01000406u || h.w[1] == 0x02000406u);
    const bool dgram = ipv4 && len >= 34 && hdr_parses(h);
    uint32_t st = (for_us ? kFrForUs : 0u) | (ipv4 ? kFrIpv4 : 0u) | (arp ? kFrArp : 0u) | (arp_ok ? kFrArpOk : 0u) |
                  (dgram ? kFrDgram : 0u);
    if constexpr (!kHop) {
      if (valid) status[i] = uint8_t(st);
    } else {
      // Router::route: ttl <= 1 dropped
      const bool fwd = dgram && h.byte(8) > 1;
      uint32_t o[5];
      hop_rewrite(h, o);
      uint32_t r_if = kNoRoute, r_hop = 0u, e0 = 0u, e1 = 0u, e2 = 0u, e3 = 0u;
      const bool routed = fwd && route_find(rt, bswap32(o[4]), r_if, r_hop);
      st |= fwd ? (routed ? 3u : 1u) : 0u;
      if (routed) {
        // send_datagram on the egress interface: its own cache, its own address
        const u32x4 out = neigh_ident(nb, r_if);
        uint32_t m_lo, m_hi;
        if ((out.y & kNeighConfigured) && neigh_find(nb, r_if, r_hop, m_lo, m_hi)) {
          st |= kFrResolved;
          e0 = m_lo << 16;                       // 0 0 dst[0] dst[1]
          e1 = (m_lo >> 16) | (m_hi << 16);      // dst[2..5]
          e2 = out.x;                            // src[0..3]
          e3 = (out.y & 0xffffu) | 0x00080000u;  // src[4] src[5] 08 00
        }
      }
      if (valid) {
        status[i] = uint8_t(st);
        if (rt_iface) rt_iface[i] = r_if;
        if (rt_hop) rt_hop[i] = r_hop;
      }
      uint32_t* rec = sw + lane64 * kRec;  // an odd stride: 64 rows on different banks
      rec[0] = e0;
      rec[1] = e1;
      rec[2] = e2;
      rec[3] = e3;
#pragma unroll
      for (int k = 0; k < 5; ++k) rec[4 + k] = fwd ? o[k] : 0u;
      wave_store<kRec>(sw, hdr_out, wbase, n, lane64);
    }
    __builtin_amdgcn_wave_barrier();  // the next pass rewrites the wave's LDS
  }
}

}  // namespace

hipError_t launch_frames(const SegSpec& sp, const RouteImg& rt, const NeighImg& nb, uint32_t in_iface,
                         const uint32_t* in_ifaces, uint32_t* hdr_out, uint8_t* status, uint32_t* iface,
                         uint32_t* next_hop, hipStream_t st) {
  const uint32_t* zpad = static_cast<const uint32_t*>(sp.zero16);
  if (hdr_out)
    hipLaunchKernelGGL(k_frame<true>, dim3(ew_blocks(sp.n)), dim3(kBlock), 0, st, sp.bytes, sp.offsets, sp.stride,
                       sp.seg_len, sp.n, in_iface, in_ifaces, hdr_out, status, zpad, rt, nb, iface, next_hop);
  else
    hipLaunchKernelGGL(k_frame<false>, dim3(ew_blocks(sp.n)), dim3(kBlock), 0, st, sp.bytes, sp.offsets,
                       sp.stride, sp.seg_len, sp.n, in_iface, in_ifaces, static_cast<uint32_t*>(nullptr), status, zpad,
                       rt, nb, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr));
  return hipGetLastError();
}

}  // namespace icsum
