// icsum_ipv4.h — IPv4 header fields and the fused IPv4 + TCP kernels
// (k_ipv4_tcp, k_ipv4_twoclass) with their launchers.
#pragma once

#include "icsum_common.h"

namespace icsum {
namespace {

// ---------------------------------------------- IPv4 header fields ------
// The first 20 wire bytes of a datagram as 5 little-endian dwords relative to
// its (possibly unaligned) start: 6 aligned dword loads + alignbyte.
struct Hdr {
  uint32_t w[5];
  __device__ __forceinline__ uint32_t byte(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }
  __device__ __forceinline__ uint32_t be16(int k) const { return (byte(k) << 8) | byte(k + 1); }
};
constexpr uint32_t kIpv4ReservedFlag = 0x00800000u;  // wire byte 6 bit 7, in w[1]: serialize() never writes it

// The aligned dword holding the byte before `end`: the last dword a load for
// a range ending at `end` (exclusive) may touch.
__device__ __forceinline__ const uint32_t* last_dword(const uint8_t* end) {
  const uint8_t* b = end - 1;
  return reinterpret_cast<const uint32_t*>(b - (reinterpret_cast<uintptr_t>(b) & 3u));
}

// Header of the datagram at p (>= 20 bytes; `last` = last_dword of its end).
// Address arithmetic stays on the global pointer p (an integer-to-pointer
// cast would turn these into flat loads, which count in both vmcnt and
// lgkmcnt and are waited for before the byte stream is issued), and every
// load is unconditional: the sixth dword, which reaches up to 3 bytes past
// byte 19 when the start is aligned, is clamped to `last`, so nothing past
// the datagram's final dword is read.
__device__ __forceinline__ Hdr load_hdr(const uint8_t* p, const uint32_t* last) {
  const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
  uint32_t d[6];
#ifdef ICSUM_BOUNDS_CHECK
  if (q + 4 > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(q + 4));
#endif
#pragma unroll
  for (int k = 0; k < 5; ++k) d[k] = q[k];
  d[5] = *(q + 5 < last ? q + 5 : last);
  Hdr h;
#pragma unroll
  for (int k = 0; k < 5; ++k) h.w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  return h;
}

// big-endian 16-bit field store: one short store when 2-byte aligned.  The
// default write-back policy: write-through (sc1), non-temporal and wider
// (16-byte, 64-byte, whole-line) stores of the same fields all measured the
// same or slower (PATCH).
__device__ __forceinline__ void store_be16(uint8_t* p, uint32_t v) {
  if ((reinterpret_cast<uintptr_t>(p) & 1u) == 0) {
    *reinterpret_cast<uint16_t*>(p) = uint16_t(((v & 0xffu) << 8) | ((v >> 8) & 0xffu));
  } else {
    p[0] = uint8_t(v >> 8);
    p[1] = uint8_t(v);
  }
}

// TCP header bytes 12..19 of a segment starting at t (>= 18 bytes present;
// `last` = last_dword of its end): tf0 = bytes 12..15, tf1 = bytes 16..19
// (bytes 18, 19 only meaningful when present).  Unconditional global loads;
// the third dword (needed only when byte 12 sits at offset 3 of its dword) is
// clamped to `last`.
__device__ __forceinline__ void load_tcp_fields(const uint8_t* t, const uint32_t* last, uint32_t& tf0,
                                                uint32_t& tf1) {
  const uint8_t* p = t + 12;
  const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
#ifdef ICSUM_BOUNDS_CHECK
  if (q + 1 > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(q + 1));
#endif
  const uint32_t d0 = q[0], d1 = q[1];
  const uint32_t d2 = *(q + 2 < last ? q + 2 : last);
  tf0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
  tf1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
}

// The same dwords unaligned (the stashed form, VRec): the six aligned dwords
// holding header bytes 0..19 at p and the three holding TCP bytes 12..19 at
// t, with their byte shifts.
__device__ __forceinline__ void load_hdr_raw(const uint8_t* p, const uint32_t* last, uint32_t* d, uint32_t& sh) {
  sh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p - sh);
#ifdef ICSUM_BOUNDS_CHECK
  if (q + 4 > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(q + 4));
#endif
#pragma unroll
  for (int k = 0; k < 5; ++k) d[k] = q[k];
  d[5] = *(q + 5 < last ? q + 5 : last);
}

__device__ __forceinline__ uint32_t tcp_shift(const uint8_t* t) {
  return uint32_t(reinterpret_cast<uintptr_t>(t + 12) & 3u);
}

// dword k (0..2) of the TCP-field window of the segment at t (the third
// clamped to `last`)
__device__ __forceinline__ uint32_t load_tcp_raw(const uint8_t* t, const uint32_t* last, uint32_t k) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(t + 12 - tcp_shift(t));
#ifdef ICSUM_BOUNDS_CHECK
  if (q + 1 > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(q + 1));
#endif
  return *(q + k < last ? q + k : last);
}

// The header dwords and the TCP fields with ONE load instruction for a lane
// group of >= 16 lanes: lane k (< 9) of the group loads header dword k (k <
// 6: the aligned window at p, the sixth clamped to `last`) or TCP-field dword
// k - 6 (the window at t + 12, the third clamped to `tlast`), the other lanes
// repeat lane 0's address.  group_hdr_take, called after the byte stream has
// been summed (loads return in order, so waiting for the stream covers this
// load too), hands every lane the nine dwords from the group's lanes —
// row_newbcast DPP for 16-lane groups (one DPP row), readlane for 64,
// ds_bpermute for 32 — and aligns them: the values of load_hdr +
// load_tcp_fields, which take 9 load instructions per lane.
struct GroupHdr {
  uint32_t v, sh, tsh;
};

template <int LPS>
__device__ __forceinline__ GroupHdr group_hdr_load(const uint8_t* p, const uint32_t* last, const uint8_t* t,
                                                   const uint32_t* tlast) {
  static_assert(LPS >= 16, "nine dwords need nine lanes of the group");
  const uint32_t k = threadIdx.x & (LPS - 1);
  GroupHdr g;
  g.sh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p - g.sh);
  const uint8_t* tp = t + 12;
  g.tsh = uint32_t(reinterpret_cast<uintptr_t>(tp) & 3u);
  const uint32_t* tq = reinterpret_cast<const uint32_t*>(tp - g.tsh);
#ifdef ICSUM_BOUNDS_CHECK
  if (k == 0 && q + 4 > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(q + 4));
  if (k == 0 && tq + 1 > tlast) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(tq + 1));
#endif
  const uint32_t* a = q;
  if (k < 5) a = q + k;
  else if (k == 5) a = q + 5 < last ? q + 5 : last;
  else if (k < 8) a = tq + (k - 6);
  else if (k == 8) a = tq + 2 < tlast ? tq + 2 : tlast;
  g.v = *a;
  return g;
}

template <int LPS>
__device__ __forceinline__ void group_hdr_take(const GroupHdr& g, Hdr& h, uint32_t& tf0, uint32_t& tf1) {
  uint32_t d[9];
  if constexpr (LPS == 16) {
#define ICS_NEWBCAST(j) d[j] = __builtin_amdgcn_update_dpp(0u, g.v, 0x150 + (j), 0xF, 0xF, false);  // row_newbcast:j
    ICS_NEWBCAST(0) ICS_NEWBCAST(1) ICS_NEWBCAST(2) ICS_NEWBCAST(3) ICS_NEWBCAST(4)
    ICS_NEWBCAST(5) ICS_NEWBCAST(6) ICS_NEWBCAST(7) ICS_NEWBCAST(8)
#undef ICS_NEWBCAST
  } else {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      if (LPS == 64)
        d[j] = __builtin_amdgcn_readlane(g.v, j);
      else
        d[j] = uint32_t(__shfl(int(g.v), int((threadIdx.x & 63u & ~(LPS - 1u)) + j), 64));
    }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) h.w[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], g.sh);
  tf0 = __builtin_amdgcn_alignbyte(d[7], d[6], g.tsh);
  tf1 = __builtin_amdgcn_alignbyte(d[8], d[7], g.tsh);
}

// IPv4Header::compute_checksum (ipv4_header.cpp:113-123): the 20 serialized
// bytes equal the wire bytes with cksum = 0 and the reserved flag bit (0x8000
// of the flags word, wire byte 6 bit 7) dropped (serialize, :78); options are
// never part of the sum.
__device__ __forceinline__ uint32_t ipv4_header_sum(const Hdr& h) {
  uint32_t e = 0, o = 0;
  acc_dword(h.w[0], e, o);
  acc_dword(h.w[1] & ~kIpv4ReservedFlag, e, o);
  acc_dword(h.w[2] & 0x0000ffffu, e, o);
  acc_dword(h.w[3], e, o);
  acc_dword(h.w[4], e, o);
  return e * 256u + o;
}

// IPv4Header::pseudo_checksum (ipv4_header.cpp:103-110); payload_length()
// wraps mod 2^16 (:89-92).
__device__ __forceinline__ uint32_t ipv4_pseudo(const Hdr& h) {
  const uint32_t hlen = h.byte(0) & 0x0fu;
  const uint32_t len = h.be16(2);
  const uint32_t src = bswap32(h.w[3]);
  const uint32_t dst = bswap32(h.w[4]);
  const uint32_t plen = (len - 4u * hlen) & 0xffffu;
  return (src >> 16) + (src & 0xffffu) + (dst >> 16) + (dst & 0xffffu) + h.byte(9) + plen;
}

// The per-datagram results of the fused kernels from its header fields, the
// TCP bytes 12..19 (tf0 / tf1, read at t0 + 12), tot = the sum of the TCP
// part [t0, e) with roles relative to t0 and its length rem = e - t0 (b16:
// the TCP part's byte 16 when rem == 17, the checksum field's only byte
// there; COMPUTE / PATCH only): IPv4Header::compute_checksum and the parse
// checks (ipv4_header.cpp:9-59, 113-123), pseudo_checksum (:103-110),
// TCPSegment::parse's verify (tcp_segment.cpp:11-18) or compute_checksum with
// the checksum field counted as 0 (:109-118), and the status bits of
// include/icsum.h.  hdr false (a datagram under 20 bytes): zeros.
struct Verdict {
  uint32_t ipc, tcv, st;
};
__device__ __forceinline__ Verdict ipv4_verdict(bool hdr, const Hdr& h, uint32_t tf0, uint32_t tf1, uint32_t tot,
                                                uint64_t rem, uint32_t b16, int mode) {
  Verdict v{0, 0, 0};
  if (hdr) {
    const uint32_t ver = h.byte(0) >> 4, hlen = h.byte(0) & 0x0fu;
    const bool hdr_ok = ver == 4 && hlen >= 5;  // ipv4_header.cpp:32-41
    v.ipc = fold_value(ipv4_header_sum(h));
    const uint32_t pseudo = ipv4_pseudo(h);
    if (h.byte(9) == 6) v.st |= 0x08;  // proto TCP
    if (rem >= 20 && ((tf0 & 0xffu) >> 4) >= 5) v.st |= 0x04;  // tcp_segment.cpp:25-65
    if (mode == 1) {
      v.tcv = fold_value(pseudo + tot);  // tcp_segment.cpp:11-18
      if (hdr_ok && v.ipc == h.be16(10)) v.st |= 0x01;  // ipv4_header.cpp:53-58
      if (v.tcv == 0) v.st |= 0x02;
    } else {
      // tcp_segment.cpp:143: the checksum field counts as 0
      uint32_t sum = pseudo + tot;
      if (rem > 16) sum -= (rem >= 18 ? tf1 & 0xffu : b16) << 8;
      if (rem > 17) sum -= (tf1 >> 8) & 0xffu;
      v.tcv = fold_value(sum);
      if (hdr_ok) v.st |= 0x01;
      if (rem >= 18) v.st |= 0x02;
    }
  }
  return v;
}

// ipv4_verdict in the claim, PATCH's two big-endian stores and the outputs
__device__ __forceinline__ void ipv4_result(uint8_t* __restrict__ dg, uint64_t s, uint64_t e, uint64_t t0, bool hdr,
                                            const Hdr& h, uint32_t tf0, uint32_t tf1, uint32_t tot, int mode,
                                            uint64_t seg, uint16_t* __restrict__ ip_ck, uint16_t* __restrict__ tcp_ck,
                                            uint8_t* __restrict__ status) {
  const uint64_t rem = e - t0;
  const uint32_t b16 = (hdr && mode != 1 && rem == 17) ? uint32_t(dg[t0 + 16]) : 0u;
  const Verdict v = ipv4_verdict(hdr, h, tf0, tf1, tot, rem, b16, mode);
  if (hdr && mode == 2) {
    store_be16(dg + s + 10, v.ipc);
    if (rem >= 18) store_be16(dg + t0 + 16, v.tcv);
  }
  if (ip_ck) ip_ck[seg] = uint16_t(v.ipc);
  if (tcp_ck) tcp_ck[seg] = uint16_t(v.tcv);
  if (status) status[seg] = uint8_t(v.st);
}

#ifdef ICSUM_STAMPS
// diagnostic build only (tools/probe/verify_stamps.hip): per block of
// k_ipv4_twoclass, s_memrealtime (100 MHz) at its start and end, and HW_ID
__device__ uint64_t g_block_stamps[1u << 16][3];
#endif

// What ipv4_result needs, kept per datagram by k_ipv4_twoclass COMPUTE /
// VERIFY, which computes the block's verdicts at its end one datagram per
// lane instead of in one lane of each group per claim: the nine dwords as
// loaded (d[0..5]: the header window, shift sh; d[6..8]: the TCP-field window,
// shift tsh; lane k < 9 of a 16-lane group writes d[k] — no broadcast, no
// alignment in the claim), the TCP part's sum and the rest packed in meta:
// hdr | sh << 2 | tsh << 4 | b16 << 8 | min(rem, 0xffff) << 16 (rem = e - t0;
// the verdict only compares it with 16..20).  44 bytes: an odd dword stride,
// conflict-free rows at the end.
struct VRec {
  uint32_t d[9], tot, meta;
};

__device__ __forceinline__ uint32_t vrec_meta(bool hdr, uint32_t sh, uint32_t tsh, uint32_t b16, uint64_t rem) {
  return uint32_t(hdr) | (sh << 2) | (tsh << 4) | (b16 << 8) | (uint32_t(rem < 0xffffu ? rem : 0xffffu) << 16);
}

__device__ __forceinline__ Verdict vrec_verdict(const VRec& r, int mode) {
  const uint32_t sh = (r.meta >> 2) & 3u, tsh = (r.meta >> 4) & 3u;
  Hdr h;
#pragma unroll
  for (int j = 0; j < 5; ++j) h.w[j] = __builtin_amdgcn_alignbyte(r.d[j + 1], r.d[j], sh);
  const uint32_t tf0 = __builtin_amdgcn_alignbyte(r.d[7], r.d[6], tsh);
  const uint32_t tf1 = __builtin_amdgcn_alignbyte(r.d[8], r.d[7], tsh);
  return ipv4_verdict((r.meta & 1u) != 0, h, tf0, tf1, r.tot, r.meta >> 16, (r.meta >> 8) & 0xffu, mode);
}

// --------------------------------------------- fused IPv4 + TCP ----------
// One datagram [s, e) per group of LPS lanes (every lane of the wave calls it:
// group sums and the wave-uniform re-sum below); `valid` false: an idle group.
// STASH: the datagram's VRec goes to stash[seg] instead of its results to
// the output rows (COMPUTE / VERIFY only).
template <int LPS, int UNROLL, bool NT, int MODE, bool STASH = false>
__device__ __forceinline__ void ipv4_item(uint8_t* __restrict__ dg, uint64_t s, uint64_t e, uint64_t seg, bool valid,
                                          uint32_t lane, int mode, uint16_t* __restrict__ ip_ck,
                                          uint16_t* __restrict__ tcp_ck, uint8_t* __restrict__ status,
                                          const uint8_t* __restrict__ zpad, const uint32_t* zlast,
                                          VRec* stash = nullptr) {
  const bool hdr = e - s >= 20;
  // Speculate the usual header length (hlen = 5): the IPv4 header dwords,
  // the TCP fields the verdict needs (data offset, checksum) and the TCP
  // byte stream are all requested before any of them returns; every lane
  // loads the header (same addresses per group, one request per wave
  // instruction), from the 32-byte zero pad when the datagram is too short.
  // A datagram with options (rare) redoes its stream below.
  uint64_t t0 = hdr ? s + 20 : e;  // TCP part: [t0, e)
  const uint32_t* last = hdr ? last_dword(dg + e) : zlast;
  Hdr h;
  uint32_t tf0 = 0, tf1 = 0;  // TCP bytes 12..15 and 16..19 (little-endian)
  const bool tcpf = hdr && e - t0 >= 18;
  GroupHdr gh{};
  [[maybe_unused]] uint32_t raw[9], sh = 0;  // STASH, one lane per datagram
  if constexpr (LPS >= 16) {
    gh = group_hdr_load<LPS>(hdr ? dg + s : zpad, last, tcpf ? dg + t0 : zpad, tcpf ? last : zlast);
  } else if constexpr (STASH) {
    load_hdr_raw(hdr ? dg + s : zpad, last, raw, sh);
    gh.tsh = tcp_shift(tcpf ? dg + t0 : zpad);
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) raw[6 + k] = load_tcp_raw(tcpf ? dg + t0 : zpad, tcpf ? last : zlast, k);
  } else {
    h = load_hdr(hdr ? dg + s : zpad, last);
    load_tcp_fields(tcpf ? dg + t0 : zpad, tcpf ? last : zlast, tf0, tf1);
  }
  uint32_t ev = 0, od = 0;
  seg_sums<LPS, UNROLL, NT, MODE>(dg, t0, e, lane, ev, od);
  uint32_t b0;  // header byte 0 (version, hlen)
  if constexpr (STASH) {
    if constexpr (LPS >= 16) {
      sh = gh.sh;
      b0 = (__builtin_amdgcn_update_dpp(0u, gh.v, 0x150, 0xF, 0xF, false) >> (8 * sh)) & 0xffu;  // row_newbcast:0
    } else {
      b0 = (raw[0] >> (8 * sh)) & 0xffu;
    }
  } else {
    if constexpr (LPS >= 16) group_hdr_take<LPS>(gh, h, tf0, tf1);
    b0 = h.byte(0);
  }
  bool redo = false;
  if (hdr) {
    uint64_t off = 4u * (b0 & 0x0fu);  // options skipped (ipv4_header.cpp:50)
    if (off < 20) off = 20;
    if (off > e - s) off = e - s;
    redo = s + off != t0;
    t0 = s + off;
    if (redo) {
      const bool f = e - t0 >= 18;
      if constexpr (STASH) {
        gh.tsh = tcp_shift(dg + t0);
        if constexpr (LPS >= 16) {
          if (lane >= 6 && lane < 9) gh.v = f ? load_tcp_raw(dg + t0, last, lane - 6) : 0u;
        } else {
#pragma unroll
          for (uint32_t k = 0; k < 3; ++k) raw[6 + k] = f ? load_tcp_raw(dg + t0, last, k) : 0u;
        }
      } else {
        tf0 = tf1 = 0;
        if (f) load_tcp_fields(dg + t0, last, tf0, tf1);
      }
    }
  }
  if (__any(redo)) {  // wave-uniform
    // The stream summed [s + 20, e); the TCP part starts at t0 = s + 4 hlen
    // (or is empty when the header claims more than the datagram holds).
    // Byte roles are by absolute address and 4 hlen - 20 is even, so the
    // options' own even / odd sums (at most 40 bytes, a few masked chunks
    // per group) come off exactly — no second pass over the payload.
    uint32_t oe = 0, oo = 0;
    if (redo) range_sums_masked<LPS, 1, false>(dg, s + 20, t0, lane, oe, oo);
    ev -= oe;
    od -= oo;
  }
  const uint32_t tot = group_sum<LPS>(combine_roles(ev, od, uint32_t(t0) & 1u));
  if constexpr (STASH) {  // the verdict later, from stash[seg]
    if (valid) {
      VRec& r = stash[seg];
      if constexpr (LPS >= 16) {
        if (lane < 9) r.d[lane] = gh.v;
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) r.d[k] = raw[k];
      }
      if (lane == LPS - 1) {
        const uint64_t rem = e - t0;
        const uint32_t b16 = (hdr && mode != 1 && rem == 17) ? uint32_t(dg[t0 + 16]) : 0u;
        r.tot = tot;
        r.meta = vrec_meta(hdr, sh, gh.tsh, b16, rem);
      }
    }
  } else if (valid && lane == LPS - 1) {
    ipv4_result(dg, s, e, t0, hdr, h, tf0, tf1, tot, mode, seg, ip_ck, tcp_ck, status);
  }
}

// datagrams [blk * groups, ...) striding by nblk blocks (block blk of nblk:
// a kernel of its own, or one batch's share of a multi-batch launch)
template <int LPS, int UNROLL, bool NT, int MODE>
__device__ __forceinline__ void ipv4_body(uint8_t* __restrict__ dg, const uint64_t* __restrict__ offsets,
                                          uint64_t stride, uint64_t dlen, uint64_t n, int mode,
                                          uint16_t* __restrict__ ip_ck, uint16_t* __restrict__ tcp_ck,
                                          uint8_t* __restrict__ status, const uint8_t* __restrict__ zpad,
                                          uint32_t blk, uint32_t nblk) {
  constexpr uint32_t kGroups = kBlock / LPS;
  const uint32_t lane = threadIdx.x & (LPS - 1);
  const uint64_t step = uint64_t(nblk) * kGroups;
  const uint32_t* const zlast = reinterpret_cast<const uint32_t*>(zpad) + 7;  // zpad: 32 zero bytes
  const uint32_t bsh = frame_shift(dg);
  dg -= bsh;
  for (uint64_t g0 = uint64_t(blk) * kGroups; g0 < n; g0 += step) {
    const uint64_t seg = g0 + threadIdx.x / LPS;
    const bool valid = seg < n;
    // offsets from a clamped index, unconditionally (a load under a divergent
    // branch is waited for at the join, before the stream below is issued)
    uint64_t s, e;
    seg_bounds(offsets, stride, dlen, valid ? seg : n - 1, s, e, bsh);
    if (!valid) e = s;
    ipv4_item<LPS, UNROLL, NT, MODE>(dg, s, e, seg, valid, lane, mode, ip_ck, tcp_ck, status, zpad, zlast);
  }
}

template <int LPS, int UNROLL, bool NT, int MODE>
__global__ __launch_bounds__(kBlock) void k_ipv4_tcp(uint8_t* __restrict__ dg,
                                                     const uint64_t* __restrict__ offsets,
                                                     uint64_t stride, uint64_t dlen, uint64_t n,
                                                     int mode, uint16_t* __restrict__ ip_ck,
                                                     uint16_t* __restrict__ tcp_ck,
                                                     uint8_t* __restrict__ status, uint32_t remap,
                                                     const uint8_t* __restrict__ zpad, Done done) {
  ipv4_body<LPS, UNROLL, NT, MODE>(dg, offsets, stride, dlen, n, mode, ip_ck, tcp_ck, status, zpad,
                                   block_order(remap), gridDim.x);
  signal_done(done);
}

// Two-class launch for receive mixes (ACKs among MTU datagrams): block b
// takes datagrams [4 SPW b, 4 SPW b + 4 SPW), wave w reads the bounds of SPW
// of them and appends each to the block's short (<= 64 bytes) or long list
// in LDS.  Wave 0 then verifies the short ones one per lane, 64 per pass,
// while the other waves — and wave 0 once its short passes are done — claim
// the long ones four at a time (16 lanes each) from an LDS counter.  A wave
// that verified both classes in turn spent a whole memory round trip on its
// short phase for a fraction of a long round's bytes; with the classes
// split over the block's waves only one wave does (½-ACK
// VERIFY of 1 M datagrams 135.5 -> 129.1 us, ¼-ACK 189.7 -> 177.8 us).
template <int SPW, int MODE_OP>  // MODE_OP: the batch's mode as a constant (only its code is built)
__global__ __launch_bounds__(kBlock) void k_ipv4_twoclass(uint8_t* __restrict__ dg, const uint64_t* __restrict__ offsets,
                                                          uint64_t stride, uint64_t dlen, uint64_t n,
                                                          int /*mode: MODE_OP*/, uint16_t* __restrict__ ip_ck,
                                                          uint16_t* __restrict__ tcp_ck, uint8_t* __restrict__ status,
                                                          const uint8_t* __restrict__ zpad, uint32_t remap) {
  constexpr uint32_t kPer = (kBlock / 64) * SPW;
  __shared__ uint64_t lst[kPer][2], sst[kPer][2];  // the block's long / short datagrams' {start, end}
  __shared__ uint32_t lseg[kPer], sseg[kPer];       // ... and their index within the block
  __shared__ uint32_t cnt[3];  // long, short, long claimed
  // COMPUTE / VERIFY: each datagram's header and TCP-field dwords as loaded
  // and its sum land in the block's records (VRec), and the block computes the
  // verdicts at its end, one datagram per lane, and writes them as three
  // coalesced rows: no header broadcast, alignment or verdict in the claims,
  // no 1-2-byte stores in claim order (stack VERIFY of 256 Ki datagrams
  // 36.22 -> 35.72 us back to back; profiles/r4_ab_twoclass_block_verdicts.jsonl).
  // PATCH stages the outputs only (its stores into the datagrams stay in the
  // claim).
  constexpr bool kStash = MODE_OP != 2;
  __shared__ VRec recs[kStash ? kPer : 1];
  __shared__ uint16_t o_ip[kStash ? 1 : kPer], o_tcp[kStash ? 1 : kPer];
  __shared__ uint8_t o_st[kStash ? 1 : kPer];
  VRec* const stash = kStash ? recs : nullptr;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t* const zlast = reinterpret_cast<const uint32_t*>(zpad) + 7;
#ifdef ICSUM_STAMPS
  const uint64_t stamp0 = __builtin_amdgcn_s_memrealtime();
#endif
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t b0 = uint64_t(block_order(remap)) * kPer;  // the block's datagrams [b0, b0 + kPer)
  const uint64_t seg = b0 + wv * SPW + (lane < SPW ? lane : 0u);
  const bool valid = seg < n && lane < SPW;
  const uint32_t bsh = frame_shift(dg);
  dg -= bsh;
  uint64_t s, e;
  seg_bounds(offsets, stride, dlen, seg < n ? seg : n - 1, s, e, bsh);
  if (!valid) e = s;
  const bool is_short = e - s <= 64;
  const uint64_t lmask = __ballot(valid && !is_short), smask = __ballot(valid && is_short);
  uint32_t lbase = 0, sbase = 0;
  if (lane == 0) {
    lbase = atomicAdd(&cnt[0], uint32_t(__builtin_popcountll(lmask)));
    sbase = atomicAdd(&cnt[1], uint32_t(__builtin_popcountll(smask)));
  }
  lbase = __builtin_amdgcn_readfirstlane(lbase);
  sbase = __builtin_amdgcn_readfirstlane(sbase);
  const uint32_t lr = __builtin_amdgcn_mbcnt_hi(uint32_t(lmask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(lmask), 0u));
  const uint32_t sr = __builtin_amdgcn_mbcnt_hi(uint32_t(smask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(smask), 0u));
  if (valid && !is_short) {
    lst[lbase + lr][0] = s;
    lst[lbase + lr][1] = e;
    lseg[lbase + lr] = uint32_t(seg - b0);
  }
  if (valid && is_short) {
    sst[sbase + sr][0] = s;
    sst[sbase + sr][1] = e;
    sseg[sbase + sr] = uint32_t(seg - b0);
  }
  __syncthreads();
  const uint32_t nlong = cnt[0], nshort = cnt[1];
  if (wv == 0)
    for (uint32_t r0 = 0; r0 < nshort; r0 += 64) {  // uniform
      const uint32_t k = r0 + lane;
      const bool mine = k < nshort;
      const uint32_t kc = mine ? k : 0u;
      const uint64_t ss = sst[kc][0], se = mine ? sst[kc][1] : ss;
      ipv4_item<1, 4, false, 0, kStash>(dg, ss, se, sseg[kc], mine, 0u, MODE_OP, o_ip, o_tcp, o_st, zpad, zlast, stash);
    }
  const uint32_t g = lane >> 4, gl = lane & 15u;
  for (;;) {
    uint32_t r0 = 0;
    if (lane == 0) r0 = atomicAdd(&cnt[2], 4u);
    r0 = __builtin_amdgcn_readfirstlane(r0);
    if (r0 >= nlong) break;  // uniform
    const uint32_t k = r0 + g;
    const bool mine = k < nlong;
    const uint32_t kc = mine ? k : 0u;
    const uint64_t ls = lst[kc][0], le = mine ? lst[kc][1] : ls;
    // 7 loads per lane: a 1500-byte datagram's line-grid span (<= 101 chunks)
    // in one pass of 112 chunks, 70 VGPRs, 7 waves / SIMD (8 loads: 76 VGPRs,
    // 6 waves; stack VERIFY 35.46 -> 34.18 us, r4_ab_twoclass_unroll7.jsonl)
    ipv4_item<16, 7, true, 3, kStash>(dg, ls, le, lseg[kc], mine, gl, MODE_OP, o_ip, o_tcp, o_st, zpad, zlast, stash);
  }
  __syncthreads();
  const uint64_t i = b0 + threadIdx.x;  // every datagram of the block was summed: its row is complete
  if (threadIdx.x < kPer && i < n) {
    uint32_t ipc, tcv, st;
    if constexpr (kStash) {
      const Verdict v = vrec_verdict(recs[threadIdx.x], MODE_OP);
      ipc = v.ipc, tcv = v.tcv, st = v.st;
    } else {
      ipc = o_ip[threadIdx.x], tcv = o_tcp[threadIdx.x], st = o_st[threadIdx.x];
    }
    if (ip_ck) ip_ck[i] = uint16_t(ipc);
    if (tcp_ck) tcp_ck[i] = uint16_t(tcv);
    if (status) status[i] = uint8_t(st);
  }
#ifdef ICSUM_STAMPS
  if (threadIdx.x == 0 && blockIdx.x < (1u << 16)) {
    uint32_t hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    g_block_stamps[blockIdx.x][0] = stamp0;
    g_block_stamps[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
    g_block_stamps[blockIdx.x][2] = hw;
  }
#endif
}

template <int LPS, int UNROLL, bool NT, int MODE>
hipError_t launch_ipv4_t(const SegSpec& sp, int mode, uint16_t* ip_ck, uint16_t* tcp_ck,
                         uint8_t* status, uint32_t max_blocks, hipStream_t st) {
  const uint32_t blocks = blocks_for(sp.n, kBlock / LPS, max_blocks);
  hipLaunchKernelGGL((k_ipv4_tcp<LPS, UNROLL, NT, MODE>), dim3(blocks), dim3(kBlock), 0, st,
                     const_cast<uint8_t*>(sp.bytes), sp.offsets, sp.stride, sp.seg_len, sp.n, mode,
                     ip_ck, tcp_ck, status, g_xcd_remap, static_cast<const uint8_t*>(sp.zero16), sp.done);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ipv4_tcp(const SegSpec& sp, int mode, uint16_t* ip_ck, uint16_t* tcp_ck,
                           uint8_t* status, Geometry g, uint32_t max_blocks, hipStream_t st) {
  hipError_t e = hipErrorInvalidValue;  // no such geometry
  for_geometry(g, [&](auto L, auto U, auto T, auto A) {
    e = launch_ipv4_t<L(), U(), T(), A()>(sp, mode, ip_ck, tcp_ck, status, max_blocks, st);
  });
  return e;
}

hipError_t launch_ipv4_twoclass(const SegSpec& sp, int mode, uint16_t* ip_ck, uint16_t* tcp_ck, uint8_t* status,
                                int spw, uint32_t remap, hipStream_t st, uint32_t lds_pad) {
  if (spw != 8 && spw != 16 && spw != 32) return hipErrorInvalidValue;
  const uint64_t blocks = twoclass_blocks(sp.n, uint64_t(spw));
  if (sp.list || blocks == 0 || blocks > kMaxGridBlocks) return hipErrorInvalidValue;
  uint8_t* const dg = const_cast<uint8_t*>(sp.bytes);
  const uint8_t* const z = static_cast<const uint8_t*>(sp.zero16);
  if (mode < 0 || mode > 2) return hipErrorInvalidValue;
#define ICS_TWO(W, M)                                                                                        \
  hipLaunchKernelGGL((k_ipv4_twoclass<W, M>), dim3(uint32_t(blocks)), dim3(kBlock), lds_pad, st, dg, sp.offsets, \
                     sp.stride, sp.seg_len, sp.n, mode, ip_ck, tcp_ck, status, z, remap)
#define ICS_TWO_M(W) \
  if (mode == 0) ICS_TWO(W, 0); else if (mode == 1) ICS_TWO(W, 1); else ICS_TWO(W, 2)
  if (spw == 8) { ICS_TWO_M(8); }
  else if (spw == 16) { ICS_TWO_M(16); }
  else { ICS_TWO_M(32); }
#undef ICS_TWO_M
#undef ICS_TWO
  return hipGetLastError();
}

}  // namespace icsum
