// icsum_hdrpass.h — what the header-only passes share (k_router_ttl,
// k_router_hdrs, k_frame, k_tcp_unwrap): the two header loads, the forward
// decision and rewrite of the router hop, and the wave-staged record store.
// Device helpers only; the kernels are in icsum_router.h, icsum_frame.h and
// icsum_unwrap.h.
#pragma once

#include "icsum_ipv4.h"

namespace icsum {
namespace {

// What one lane of a wave wrote to LDS, every lane of the wave may read
// afterwards (and the other way round before a rewrite).
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One rule for an item's length: offsets are monotone by the caller's
// contract (the bounds-checked build reports a breach in seg_bounds); where
// they are not, the item is empty and reads the zero pad.
__device__ __forceinline__ uint64_t item_len(uint64_t s, uint64_t e) { return e >= s ? e - s : 0; }

// ------------------------------------------- 64 items per wave, in rows ---
// Load: an item's first 36 bytes lie in at most four of the aligned 16-byte
// blocks that hold it.  Four lanes per item, lane j loading block j with ONE
// dwordx4 load clamped at the item's last block (an item below kMin bytes, or
// one past the batch, reads the zero pad): four load instructions per 64
// items, each touching 16 items with 64 neighbouring bytes, and nothing
// outside the blocks that hold the item is read.  The blocks go to LDS, one
// 17-dword row per item: LDS takes any dword address, and the odd row length
// keeps 64 rows on different banks.  Clamped blocks are never interpreted:
// the callers' decisions read only bytes their length checks have shown to
// exist.  `base` is 16-byte aligned (moved down by bsh), so block bounds are
// multiples of 16 in its frame; the wave's items are [wbase, wbase + 64).
constexpr uint32_t kRow = 17, kRowsPerWave = 64;

template <uint32_t kMin>
__device__ __forceinline__ void rows_load(const uint8_t* __restrict__ base, const uint64_t* __restrict__ offsets,
                                          uint64_t stride, uint64_t len, uint64_t n, uint32_t bsh, uint64_t wbase,
                                          uint32_t lane64, const uint32_t* __restrict__ zpad, uint32_t* rw) {
  const uint32_t blk = lane64 & 3u;
  // pass q brings items wbase + 16 q .. + 15, four lanes each
  u32x4 v[4];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint64_t j = wbase + 16u * q + (lane64 >> 2);
    uint64_t s, e;
    seg_bounds(offsets, stride, len, j < n ? j : n - 1, s, e, bsh);
    const bool ok = j < n && item_len(s, e) >= kMin;
    const uint64_t a0 = s & ~uint64_t(15), alast = (e - 1) & ~uint64_t(15);
    const uint64_t at = a0 + 16u * blk < alast ? a0 + 16u * blk : alast;
    const u32x4* src = ok ? reinterpret_cast<const u32x4*>(base + at) : reinterpret_cast<const u32x4*>(zpad) + blk;
#ifdef ICSUM_BOUNDS_CHECK
    if (ok) ICS_CHECK16(src, base + a0, base + ((e + 15) & ~uint64_t(15)));
#endif
    v[q] = *src;
  }
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    uint32_t* row = rw + (16u * q + (lane64 >> 2)) * kRow + 4u * blk;
    row[0] = v[q].x;
    row[1] = v[q].y;
    row[2] = v[q].z;
    row[3] = v[q].w;
  }
  wave_lds_sync();
}

// Parse side, ONE lane per item: lane l reads the ten dwords of row l from
// the item's start dword on and aligns them to the item's start s (alignbyte
// by its low two bits): f[k] = item bytes 4k .. 4k + 3.  ok false (the row
// holds the zero pad): zeros.
__device__ __forceinline__ void row_take(const uint32_t* rw, uint32_t lane64, bool ok, uint64_t s, uint32_t f[9]) {
  const uint32_t o = ok ? uint32_t(s & 15u) >> 2 : 0u, sh = ok ? uint32_t(s & 3u) : 0u;
  uint32_t d[10];
#pragma unroll
  for (int w = 0; w < 10; ++w) d[w] = rw[lane64 * kRow + o + w];  // o + 9 <= 12
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
}

// -------------------------------------------- two lanes per datagram ------
// Lane 0 of a pair loads header dwords 0, 2, 4 and lane 1 dwords 1, 3, 5, so
// each wave instruction touches 32 header lines with two neighbouring dwords
// each instead of 64 lines with one (one lane loading all six dwords: six
// instructions of 64 lines; the memory side then saw ~1.9 128-byte read
// requests per datagram for ~1.16 lines of header).  Measured
// (git 7692616:tools/probe/router_probe.hip, profiles/r2_router_probe.jsonl): 1 M x 1500 B
// 59.8 -> 57.3 us; the read-only floor of the same headers is 35-41 us, the
// rest is the scattered 8-byte write-back of every forwarded header.
// Datagram i of [s, e) in the frame of dg; both lanes of the pair get its
// header and the start's byte shift.  A datagram too short for a header (or
// an idle pair, i >= n) reads the zero pad and returns false.  Every lane of
// the wave calls it (shuffles).
__device__ __forceinline__ bool pair_hdr_load(const uint8_t* dg, const uint64_t* __restrict__ offsets,
                                              uint64_t stride, uint64_t dlen, uint64_t n, uint32_t bsh, uint64_t i,
                                              const uint32_t* __restrict__ zpad, Hdr& h, uint32_t& sh, uint64_t& s) {
  const uint32_t lane = threadIdx.x & 1u;
  uint64_t e;
  seg_bounds(offsets, stride, dlen, i < n ? i : n - 1, s, e, bsh);
  const bool hdr = i < n && item_len(s, e) >= 20;
  const uint8_t* p = dg + s;
  sh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
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
  // all three loads are requested before the first shuffle waits for one (left
  // to the scheduler, k_router_ttl issued a load only after an earlier one had
  // returned: profiles/hdrpass_refactor.jsonl, the in-place rows)
  __builtin_amdgcn_sched_barrier(0);
  const int pair = int(threadIdx.x & 63u & ~1u);
  uint32_t d[6];
#pragma unroll
  for (int w = 0; w < 6; ++w) d[w] = uint32_t(__shfl(int(mine[w / 2]), pair + (w & 1), 64));
#pragma unroll
  for (int k = 0; k < 5; ++k) h.w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  return hdr;
}

// ------------------------------------------------------ the router hop ----
// NetworkInterface::recv_frame's parse (network_interface.cpp:51;
// ipv4_header.cpp:32-41, :53-58): version 4, hlen >= 5, header checksum good.
__device__ __forceinline__ bool hdr_parses(const Hdr& h) {
  return (h.byte(0) >> 4) == 4 && (h.byte(0) & 0x0fu) >= 5 && fold_value(ipv4_header_sum(h)) == h.be16(10);
}

// Router::route on a header that parses and whose ttl is above 1: ttl-- and
// compute_checksum() (router.cpp:39-66), then what serialize() makes of it
// (ipv4_header.cpp:62-86: options never written, the reserved flag bit
// dropped).  o: the 20 forwarded header bytes.
__device__ __forceinline__ void hop_rewrite(Hdr h, uint32_t o[5]) {
  h.w[2] = (h.w[2] & ~0xffu) | ((h.byte(8) - 1) & 0xffu);
  const uint32_t c = fold_value(ipv4_header_sum(h));
  o[0] = h.w[0];
  o[1] = h.w[1] & ~kIpv4ReservedFlag;
  o[2] = (h.w[2] & 0x0000ffffu) | ((c >> 8) << 16) | ((c & 0xffu) << 24);  // ttl - 1, protocol, checksum
  o[3] = h.w[3];
  o[4] = h.w[4];
}

// ------------------------------------------------ wave-staged records -----
// The wave has staged kPer records of kRec dwords in sw, those of items
// [wbase, wbase + kPer): they go out as consecutive dwords of `out`, cut at
// item n.  The caller's loop ends with a wave_barrier before sw is rewritten.
template <uint32_t kRec, uint32_t kPer = kRowsPerWave>
__device__ __forceinline__ void wave_store(const uint32_t* sw, uint32_t* __restrict__ out, uint64_t wbase, uint64_t n,
                                           uint32_t lane64) {
  wave_lds_sync();
  const uint64_t cnt = wbase < n ? (n - wbase < kPer ? n - wbase : kPer) : 0;
#pragma unroll
  for (uint32_t j = 0; j < (kPer * kRec + 63u) / 64u; ++j) {
    const uint32_t t = j * 64u + lane64;
    if (t < cnt * kRec) out[wbase * kRec + t] = sw[t];
  }
}

}  // namespace
}  // namespace icsum
