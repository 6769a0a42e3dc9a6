// icsum_wrap.h — the device-side wrap_tcp_in_ip (k_tcp_wrap, k_tcp_hdr,
// wrap_header) and its launchers.
#pragma once

#include "icsum_common.h"

namespace icsum {
namespace {

// ------------------------------------------- device-side wrap (f2) -------
// TCPOverIPv4Adapter::wrap_tcp_in_ip (tcp_over_ip.cpp:69-88) for a batch:
// datagram i = [40 header bytes][payload], the payload already in place (laid
// once at its final offset by the caller).  One pass per datagram sums the
// payload; the lanes of its group then write the serialized IPv4 header
// (ipv4_header.cpp:62-86: ver 4, hlen 5, tos 0, len, id, DF, ttl, proto 6,
// checksum, src, dst) and TCP header (tcp_segment.cpp:76-106: ports, seqno,
// ackno, data offset 5, flags, window, checksum, urgent 0) with both
// checksums: TCPSegment::compute_checksum seeded with the pseudo sum (len =
// 40 + payload, uint16 like the reference's field), then
// IPv4Header::compute_checksum.  hdr_out != nullptr: the 40 bytes go to
// hdr_out[40 i ..] instead of in place (the host-memory path copies only them
// back).  Datagrams shorter than 40 bytes are left as they are.
template <int LPS, int UNROLL, bool NT, int MODE, bool SUMS>
__global__ __launch_bounds__(kBlock) void k_tcp_wrap(uint8_t* __restrict__ dg,
                                                     const uint64_t* __restrict__ offsets,
                                                     uint64_t stride, uint64_t dlen, uint64_t n,
                                                     const TcpMsg* __restrict__ msgs,
                                                     uint32_t* __restrict__ hdr_out,
                                                     uint16_t* __restrict__ ip_ck,
                                                     uint16_t* __restrict__ tcp_ck, uint32_t remap,
                                                     int payload_only, uint32_t* __restrict__ sums, Done done) {
  constexpr uint32_t kGroups = kBlock / LPS;
  const uint32_t lane = threadIdx.x & (LPS - 1);
  const uint64_t step = uint64_t(gridDim.x) * kGroups;
  const uint32_t bsh = frame_shift(dg);
  dg -= bsh;
  for (uint64_t g0 = uint64_t(block_order(remap)) * kGroups; g0 < n; g0 += step) {
    const uint64_t seg = g0 + threadIdx.x / LPS;
    const bool valid = seg < n;
    const uint64_t idx = valid ? seg : n - 1;  // clamped index: every load unconditional
    uint64_t s, e;
    seg_bounds(offsets, stride, dlen, idx, s, e, bsh);
    if (!valid) e = s;
    // payload_only: segment i is the payload alone, its headers go to hdr_out
    const bool ok = valid && (payload_only || e - s >= 40);
    TcpMsg m{};
    if (!SUMS) m = msgs[idx];  // same address across the group: one request per wave instruction
    const uint64_t p0 = ok ? (payload_only ? s : s + 40) : e;  // payload [p0, e)
    uint32_t ev = 0, od = 0;
    seg_sums<LPS, UNROLL, NT, MODE>(dg, p0, e, lane, ev, od);
    uint32_t tot = group_sum<LPS>(combine_roles(ev, od, uint32_t(p0) & 1u));
    if (SUMS) {  // pass 1 of the two-pass wrap: the payload sums only (k_tcp_hdr writes the headers)
      if (valid && lane == LPS - 1) sums[seg] = tot;
      continue;
    }
    if (LPS > 16) tot = __shfl(tot, int((threadIdx.x & 63u) | (LPS - 1)) & 63, 64);  // to every lane of the group
    // both checksums (16-bit big-endian words of the serialized headers)
    const uint32_t len = uint32_t(e - p0 + 40) & 0xffffu;  // IPv4Header::len is uint16
    const uint32_t ttl_proto = (uint32_t(m.ttl) << 8) | 6u;  // big-endian word 4 of the IPv4 header
    const uint32_t addr = (m.src >> 16) + (m.src & 0xffffu) + (m.dst >> 16) + (m.dst & 0xffffu);
    const uint32_t ipc = fold_value(0x4500u + len + m.id + 0x4000u + ttl_proto + addr);
    const uint32_t pseudo = addr + 6u + ((len - 20u) & 0xffffu);  // ipv4_header.cpp:103-110
    const uint32_t thdr = uint32_t(m.sport) + m.dport + (m.seqno >> 16) + (m.seqno & 0xffffu) + (m.ackno >> 16) +
                          (m.ackno & 0xffffu) + (0x5000u | m.flags) + m.window;
    const uint32_t tcv = fold_value(pseudo + thdr + tot);
    // the 10 header dwords over the group's lanes (groups of 4 or 8 lanes
    // write two or three each)
    auto be16 = [](uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); };
    uint8_t* h = dg + s;
    const bool aligned = (reinterpret_cast<uintptr_t>(h) & 3u) == 0;
    for (uint32_t k = lane; ok && k < 10; k += LPS) {
      uint32_t w;  // dword k of the 40 wire bytes, little-endian
      switch (k) {
        case 0: w = 0x45u | (be16(len) << 16); break;
        case 1: w = be16(m.id) | (0x40u << 16); break;
        case 2: w = uint32_t(m.ttl) | (6u << 8) | (be16(ipc) << 16); break;  // ttl, proto, checksum
        case 3: w = bswap32(m.src); break;
        case 4: w = bswap32(m.dst); break;
        case 5: w = be16(m.sport) | (be16(m.dport) << 16); break;
        case 6: w = bswap32(m.seqno); break;
        case 7: w = bswap32(m.ackno); break;
        case 8: w = 0x50u | (uint32_t(m.flags) << 8) | (be16(m.window) << 16); break;
        default: w = be16(tcv); break;  // checksum, urgent pointer 0
      }
      if (hdr_out)
        hdr_out[seg * 10 + k] = w;
      else if (aligned)
        reinterpret_cast<uint32_t*>(h)[k] = w;
      else {
#pragma unroll
        for (int b = 0; b < 4; ++b) h[4 * k + b] = uint8_t(w >> (8 * b));
      }
    }
    if (valid && lane == 0) {
      if (ip_ck) ip_ck[seg] = ok ? uint16_t(ipc) : uint16_t(0);
      if (tcp_ck) tcp_ck[seg] = ok ? uint16_t(tcv) : uint16_t(0);
    }
  }
  signal_done(done);
}

// The 40 wire bytes wrap_tcp_in_ip puts in front of a payload of plen bytes
// whose sum (roles relative to the payload start) is tot, from the message
// record (ics_tcp_msg as dwords: a = src, dst, seqno, ackno; r4 = sport |
// dport << 16; r5 = window | flags << 16 | ttl << 24; r6 = id): the IPv4
// header (ipv4_header.cpp:62-86) and TCP header (tcp_segment.cpp:76-106) as
// 10 little-endian dwords into w, with both checksums —
// TCPSegment::compute_checksum seeded with the pseudo sum, then
// IPv4Header::compute_checksum (tcp_over_ip.cpp:83-84) — also into ipc / tcv.
__device__ __forceinline__ void wrap_header(const u32x4& a, uint32_t r4, uint32_t r5, uint32_t r6, uint64_t plen,
                                            uint32_t tot, uint32_t* w, uint32_t& ipc, uint32_t& tcv) {
  auto be16 = [](uint32_t v) { return ((v & 0xffu) << 8) | ((v >> 8) & 0xffu); };
  const uint32_t sport = r4 & 0xffffu, dport = r4 >> 16, window = r5 & 0xffffu;
  const uint32_t flags = (r5 >> 16) & 0xffu, ttl = r5 >> 24;
  const uint32_t len = uint32_t(plen + 40) & 0xffffu;  // IPv4Header::len is uint16
  const uint32_t addr = (a.x >> 16) + (a.x & 0xffffu) + (a.y >> 16) + (a.y & 0xffffu);
  ipc = fold_value(0x4500u + len + r6 + 0x4000u + ((ttl << 8) | 6u) + addr);
  const uint32_t pseudo = addr + 6u + ((len - 20u) & 0xffffu);  // ipv4_header.cpp:103-110
  const uint32_t thdr = sport + dport + (a.z >> 16) + (a.z & 0xffffu) + (a.w >> 16) + (a.w & 0xffffu) +
                        (0x5000u | flags) + window;
  tcv = fold_value(pseudo + thdr + tot);
  w[0] = 0x45u | (be16(len) << 16);
  w[1] = be16(r6) | (0x40u << 16);                     // id, DF
  w[2] = ttl | (6u << 8) | (be16(ipc) << 16);          // ttl, proto, checksum
  w[3] = bswap32(a.x);
  w[4] = bswap32(a.y);
  w[5] = be16(sport) | (be16(dport) << 16);
  w[6] = bswap32(a.z);
  w[7] = bswap32(a.w);
  w[8] = 0x50u | (flags << 8) | (be16(window) << 16);  // data offset 5, flags, window
  w[9] = be16(tcv);                                    // checksum, urgent pointer 0
}

// Pass 2 of the device wrap when the headers go to an array of their own and
// the batch is large (in place, and for short batches, the one-pass k_tcp_wrap
// above is faster): the headers of 64 datagrams per wave from their 28-byte
// records and the payload sums pass 1 left in `sums`.  Lane d builds datagram
// d's 10 dwords and both checksums (the same arithmetic as k_tcp_wrap); LDS
// turns them around so each store instruction writes 64 consecutive header
// dwords — 256 contiguous bytes of hdr_out, or the headers of 6-7
// neighbouring datagrams in place.  Header stores inside the payload stream
// cost ≈40 ps per datagram apart and ≈85 ps in place
// (profiles/r2_ab_wrap_variant.jsonl); here the apart ones are a
// 14 us launch of their own per 1 M datagrams.
__global__ __launch_bounds__(kBlock) void k_tcp_hdr(uint8_t* __restrict__ dg,
                                                    const uint64_t* __restrict__ offsets, uint64_t stride,
                                                    uint64_t dlen, uint64_t n, const TcpMsg* __restrict__ msgs,
                                                    const uint32_t* __restrict__ sums,
                                                    uint32_t* __restrict__ hdr_out, uint16_t* __restrict__ ip_ck,
                                                    uint16_t* __restrict__ tcp_ck, int payload_only, Done done) {
  __shared__ uint32_t stage[kBlock / 64][64 * 10];  // 10 KiB: each wave's 640 header dwords
  const uint32_t lane64 = threadIdx.x & 63u;
  uint32_t* const sw = stage[threadIdx.x >> 6];
  const uint32_t bsh = frame_shift(dg);
  dg -= bsh;
  for (uint64_t b0 = uint64_t(blockIdx.x) * kBlock; b0 < n; b0 += uint64_t(gridDim.x) * kBlock) {
    const uint64_t base = b0 + (threadIdx.x & ~63u);  // the wave's first datagram
    if (base >= n) continue;                          // wave-uniform
    const uint64_t i = base + lane64;
    const bool valid = i < n;
    const uint64_t idx = valid ? i : n - 1;
    uint64_t s, e;
    seg_bounds(offsets, stride, dlen, idx, s, e, bsh);
    const bool ok = valid && (payload_only || e - s >= 40);
    // the record as dwordx4 + dwordx3 (ics_tcp_msg: src, dst, seqno, ackno;
    // sport | dport << 16; window | flags << 16 | ttl << 24; id)
    const uint32_t* r = reinterpret_cast<const uint32_t*>(msgs + idx);
    u32x4 a;
    __builtin_memcpy(&a, r, 16);
    const uint32_t r4 = r[4], r5 = r[5], r6 = r[6] & 0xffffu;
    const uint32_t tot = sums[idx];
    const uint64_t p0 = payload_only ? s : s + 40;
    uint32_t ipc, tcv;
    wrap_header(a, r4, r5, r6, e - p0, tot, sw + lane64 * 10, ipc, tcv);
    if (valid) {
      if (ip_ck) ip_ck[i] = ok ? uint16_t(ipc) : uint16_t(0);
      if (tcp_ck) tcp_ck[i] = ok ? uint16_t(tcv) : uint16_t(0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // store j: the wave's header dword t = 64 j + lane64 = dword t % 10 of datagram t / 10
    const int s_lo = int(uint32_t(s)), s_hi = int(uint32_t(s >> 32)), ok_i = int(ok);
#pragma unroll
    for (uint32_t j = 0; j < 10; ++j) {
      const uint32_t t = j * 64 + lane64, d = t / 10, k = t - d * 10;
      const uint32_t w = sw[t];
      const bool dok = __shfl(ok_i, int(d), 64) != 0;
      if (hdr_out) {
        if (dok) hdr_out[base * 10 + t] = w;
      } else {
        const uint64_t ds = (uint64_t(uint32_t(__shfl(s_hi, int(d), 64))) << 32) | uint32_t(__shfl(s_lo, int(d), 64));
        uint8_t* h = dg + ds + 4 * k;
        if (dok) {
          if ((reinterpret_cast<uintptr_t>(h) & 3u) == 0)
            *reinterpret_cast<uint32_t*>(h) = w;
          else {
#pragma unroll
            for (int b = 0; b < 4; ++b) h[b] = uint8_t(w >> (8 * b));
          }
        }
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next step rewrites sw
  }
  signal_done(done);
}

template <int LPS, int UNROLL, bool NT, int MODE>
hipError_t launch_wrap_t(const SegSpec& sp, const TcpMsg* msgs, uint32_t* hdr_out, uint16_t* ip_ck,
                         uint16_t* tcp_ck, bool payload_only, uint32_t* sums, uint32_t max_blocks, hipStream_t st) {
  const uint32_t blocks = blocks_for(sp.n, kBlock / LPS, max_blocks);
  if (sums)
    hipLaunchKernelGGL((k_tcp_wrap<LPS, UNROLL, NT, MODE, true>), dim3(blocks), dim3(kBlock), 0, st,
                       const_cast<uint8_t*>(sp.bytes), sp.offsets, sp.stride, sp.seg_len, sp.n, msgs, hdr_out,
                       ip_ck, tcp_ck, g_xcd_remap, int(payload_only), sums, Done{});  // k_tcp_hdr completes
  else
    hipLaunchKernelGGL((k_tcp_wrap<LPS, UNROLL, NT, MODE, false>), dim3(blocks), dim3(kBlock), 0, st,
                       const_cast<uint8_t*>(sp.bytes), sp.offsets, sp.stride, sp.seg_len, sp.n, msgs, hdr_out,
                       ip_ck, tcp_ck, g_xcd_remap, int(payload_only), sums, sp.done);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_tcp_wrap(const SegSpec& sp, const TcpMsg* msgs, uint32_t* hdr_out, uint16_t* ip_ck,
                           uint16_t* tcp_ck, bool payload_only, uint32_t* sums, Geometry g, uint32_t max_blocks,
                           hipStream_t st) {
  if (sp.n == 0) return hipSuccess;
  if (payload_only && !hdr_out) return hipErrorInvalidValue;
  hipError_t e = hipErrorInvalidValue;  // no such geometry
  for_geometry(g, [&](auto L, auto U, auto T, auto A) {
    e = launch_wrap_t<L(), U(), T(), A()>(sp, msgs, hdr_out, ip_ck, tcp_ck, payload_only, sums, max_blocks, st);
  });
  if (e != hipSuccess || !sums) return e;
  return launch_tcp_hdr(sp, msgs, sums, hdr_out, ip_ck, tcp_ck, payload_only, st);
}

hipError_t launch_tcp_hdr(const SegSpec& sp, const TcpMsg* msgs, const uint32_t* sums, uint32_t* hdr_out,
                          uint16_t* ip_ck, uint16_t* tcp_ck, bool payload_only, hipStream_t st) {
  if (sp.n == 0) return hipSuccess;
  const uint64_t blocks = (sp.n + kBlock - 1) / kBlock;  // one datagram per lane
  hipLaunchKernelGGL(k_tcp_hdr, dim3(uint32_t(blocks < (uint64_t(1) << 22) ? blocks : (uint64_t(1) << 22))),
                     dim3(kBlock), 0, st, const_cast<uint8_t*>(sp.bytes), sp.offsets, sp.stride, sp.seg_len, sp.n,
                     msgs, sums, hdr_out, ip_ck, tcp_ck, int(payload_only), sp.done);
  return hipGetLastError();
}

}  // namespace icsum
