// icsum_checksum.h — the checksum kernels (a1-a4): one lane group per segment
// (k_checksum), small, tiny, two-class, dense and binned launches, k_fold, the
// geometry choice and their launchers.
#pragma once

#include "icsum_binning.h"

namespace icsum {
namespace {

// ------------------------------------------------------------ a1-a4 -------
// `init` / `odd` are never null here: an absent array is replaced by a
// 16-byte zero buffer read with index step 0 (init_step / odd_step).
// (block blk of nblk: a kernel of its own, or one bin's share of k_checksum_bins)
template <int LPS, int UNROLL, bool NT, int MODE, int OUT>
__device__ __forceinline__ void checksum_body(const uint8_t* __restrict__ bytes, const SegSrc& src,
                                              const uint32_t* __restrict__ init, uint32_t init_step,
                                              const uint8_t* __restrict__ odd, uint32_t odd_step,
                                              void* __restrict__ out, uint64_t n, uint32_t blk, uint32_t nblk) {
  constexpr uint32_t kGroups = kBlock / LPS;
  const uint32_t lane = threadIdx.x & (LPS - 1);
  const Work w = resolve(src, n);
  auto item = [&](uint64_t gi, const ItemMeta& m) {
    uint64_t seg, s, e;
    src_decode(src, w, gi, m, seg, s, e);
    const bool valid = gi < w.items;
    // per-segment metadata is requested together with the byte stream, so a
    // wave waits on memory once (the leader lane folds it in at the end)
    // (unconditional loads from a clamped index: a load under a divergent
    // branch would make the compiler wait for it at the join)
    const bool leader = valid && lane == LPS - 1;
    const uint64_t cseg = seg;  // 0 for idle lanes (n >= 1)
    const uint32_t i0 = init[cseg * init_step];
    // a high byte at the start unless the start is odd XOR parity_ was already odd
    const uint32_t swap = (uint32_t(s) ^ uint32_t(odd[cseg * odd_step])) & 1u;
    uint32_t ev = 0, od = 0;
    seg_sums<LPS, UNROLL, NT, MODE>(bytes, s, e, lane, ev, od);
    const uint32_t tot = group_sum<LPS>(combine_roles(ev, od, swap));
    if (leader) {
      const uint32_t sum = i0 + tot;
      if (OUT == 0)
        static_cast<uint16_t*>(out)[seg] = fold_value(sum);
      else
        static_cast<uint32_t*>(out)[seg] = sum;
    }
  };
  // the pass bound is uniform per block, so every lane reaches the DPP sums
  for (uint64_t g0 = uint64_t(blk) * kGroups; g0 < w.items; g0 += uint64_t(nblk) * kGroups) {
    const uint64_t gi = g0 + threadIdx.x / LPS;
    item(gi, src_fetch(src, w, gi, n));
  }
}

// Small segments (a few 16-byte chunks): a lane group owns SEGS segments per
// pass and issues the first LPS*UNROLL chunk loads of ALL of them before any
// is consumed, so a wave keeps SEGS times the bytes in flight of the
// one-segment kernel (small segments are latency-bound, not VALU-bound).
// Instruction k of a wave covers 64/LPS consecutive segments, i.e. one
// contiguous 1 KiB run for 64-byte segments.  Every slot is masked to its
// segment (range_sums_masked semantics); a segment longer than LPS*UNROLL
// chunks finishes in a loop.  Absent per-segment arrays: zero16 + step 0.
template <int LPS, int UNROLL, int SEGS, int OUT>
__device__ __forceinline__ void checksum_small_body(const uint8_t* __restrict__ bytes, const SegSrc& src,
                                                    const uint32_t* __restrict__ init, uint32_t init_step,
                                                    const uint8_t* __restrict__ odd, uint32_t odd_step,
                                                    const u32x4* __restrict__ zero16, void* __restrict__ out,
                                                    uint64_t n, uint32_t blk, uint32_t nblk) {
  constexpr uint32_t kGroups = kBlock / LPS;
  constexpr uint32_t kSlots = LPS * UNROLL;
  const uint32_t lane = threadIdx.x & (LPS - 1);
  const uint32_t group = threadIdx.x / LPS;
  const Work w = resolve(src, n);  // never a whole-batch run (the last bin is not small)
  for (uint64_t g0 = uint64_t(blk) * kGroups * SEGS; g0 < w.items; g0 += uint64_t(nblk) * kGroups * SEGS) {
    uint64_t s[SEGS], span[SEGS], segk[SEGS];
    bool validk[SEGS];
    uint32_t nch[SEGS], i0[SEGS], swap[SEGS];
    u32x4 v[SEGS][UNROLL];
#pragma unroll
    for (int k = 0; k < SEGS; ++k) {
      const uint64_t gi = g0 + uint64_t(k) * kGroups + group;
      validk[k] = gi < w.items;
      uint64_t e;
      src_locate(src, w, gi, n, segk[k], s[k], e);
      const uint64_t a0 = s[k] & ~uint64_t(15);
      span[k] = e > s[k] ? e - a0 : 0;
      nch[k] = uint32_t((span[k] + 15) >> 4);
      const uint64_t cseg = segk[k];  // 0 for idle lanes (n >= 1)
      i0[k] = init[cseg * init_step];
      swap[k] = (uint32_t(s[k]) ^ uint32_t(odd[cseg * odd_step])) & 1u;
      const u32x4* p = reinterpret_cast<const u32x4*>(bytes + a0);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const uint32_t cc = lane + uint32_t(u * LPS);
        // unconditional load from a valid address (empty segment -> zero16)
        const u32x4* q = nch[k] ? p + (cc < nch[k] ? cc : nch[k] - 1) : zero16;
        if (nch[k]) ICS_CHECK16(q, bytes + a0, bytes + a0 + (uint64_t(nch[k]) << 4));
        v[k][u] = __builtin_nontemporal_load(q);
      }
    }
#pragma unroll
    for (int k = 0; k < SEGS; ++k) {
      uint32_t ev = 0, od = 0;
      const uint32_t lo0 = uint32_t(s[k]) & 15u;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const uint32_t cc = lane + uint32_t(u * LPS);
        const uint64_t at = uint64_t(cc) << 4;
        const uint32_t lo = cc == 0 ? lo0 : 0u;
        const uint32_t hi = at >= span[k] ? 0u : (span[k] - at >= 16 ? 16u : uint32_t(span[k] - at));
        acc_chunk(v[k][u] & byte_range_mask(lo, hi), ev, od);
      }
      if (nch[k] > kSlots) {  // long segment: the rest, masked (rare in this kernel's range)
        const u32x4* p = reinterpret_cast<const u32x4*>(bytes + (s[k] & ~uint64_t(15)));
        for (uint32_t cc = lane + kSlots; cc < nch[k]; cc += LPS) {
          const uint64_t at = uint64_t(cc) << 4;
          const uint32_t hi = span[k] - at >= 16 ? 16u : uint32_t(span[k] - at);
          ICS_CHECK16(p + cc, reinterpret_cast<const uint8_t*>(p),
                      reinterpret_cast<const uint8_t*>(p) + (uint64_t(nch[k]) << 4));
          acc_chunk(__builtin_nontemporal_load(p + cc) & byte_range_mask(0u, hi), ev, od);
        }
      }
      const uint32_t tot = group_sum<LPS>(combine_roles(ev, od, swap[k]));
      const uint64_t seg = segk[k];
      if (validk[k] && lane == LPS - 1) {
        const uint32_t sum = i0[k] + tot;
        if (OUT == 0)
          static_cast<uint16_t*>(out)[seg] = fold_value(sum);
        else
          static_cast<uint32_t*>(out)[seg] = sum;
      }
    }
  }
}

// Tiny segments (ACK-sized TCP segments, <= 4 chunks): ONE lane per segment.
// The wave's offsets load is one coalesced 512-byte read, each lane then
// issues its segment's (up to) four 16-byte loads at once — neighbouring
// lanes' segments share lines, so the loads keep the default cache policy
// and a line a neighbour also reads comes from L2 — and masks them to the
// segment.  A longer segment finishes its remaining chunks in a loop (rare
// in this kernel's range: the plans send it batches of short segments).
// Absent per-segment arrays: zero16 + step 0.
template <int OUT>
__device__ __forceinline__ void checksum_tiny_body(const uint8_t* __restrict__ bytes, const SegSrc& src,
                                                   const uint32_t* __restrict__ init, uint32_t init_step,
                                                   const uint8_t* __restrict__ odd, uint32_t odd_step,
                                                   const u32x4* __restrict__ zero16, void* __restrict__ out,
                                                   uint64_t n, uint32_t blk, uint32_t nblk) {
  constexpr int kSlots = 4;
  const Work w = resolve(src, n);
  for (uint64_t g0 = uint64_t(blk) * kBlock; g0 < w.items; g0 += uint64_t(nblk) * kBlock) {
    const uint64_t gi = g0 + threadIdx.x;
    uint64_t seg, s, e;
    src_locate(src, w, gi, n, seg, s, e);
    const uint64_t a0 = s & ~uint64_t(15);
    const uint64_t span = e > s ? e - a0 : 0;
    const uint32_t nch = uint32_t((span + 15) >> 4);
    const u32x4* __restrict__ p = reinterpret_cast<const u32x4*>(bytes + a0);
    u32x4 v[kSlots];
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      // unconditional load from a valid address (empty segment -> zero16)
      const u32x4* q = nch ? p + (uint32_t(u) < nch ? uint32_t(u) : nch - 1) : zero16;
      if (nch) ICS_CHECK16(q, bytes + a0, bytes + a0 + (uint64_t(nch) << 4));
      v[u] = *q;
    }
    const uint32_t i0 = init[seg * init_step];
    const uint32_t swap = (uint32_t(s) ^ uint32_t(odd[seg * odd_step])) & 1u;
    uint32_t ev = 0, od = 0;
#pragma unroll
    for (int u = 0; u < kSlots; ++u) {
      const uint64_t at = uint64_t(u) << 4;
      const uint32_t lo = u == 0 ? uint32_t(s) & 15u : 0u;
      const uint32_t hi = at >= span ? 0u : (span - at >= 16 ? 16u : uint32_t(span - at));
      acc_chunk(v[u] & byte_range_mask(lo, hi), ev, od);
    }
    for (uint32_t c = kSlots; c < nch; ++c) {  // longer segments
      const uint64_t at = uint64_t(c) << 4;
      const uint32_t hi = span - at >= 16 ? 16u : uint32_t(span - at);
      ICS_CHECK16(p + c, bytes + a0, bytes + a0 + (uint64_t(nch) << 4));
      acc_chunk(p[c] & byte_range_mask(0u, hi), ev, od);
    }
    if (gi < w.items) {
      const uint32_t sum = i0 + combine_roles(ev, od, swap);
      if (OUT == 0)
        static_cast<uint16_t*>(out)[seg] = fold_value(sum);
      else
        static_cast<uint32_t*>(out)[seg] = sum;
    }
  }
}

template <int LPS, int UNROLL, bool NT, int MODE, int OUT>
__device__ __forceinline__ void checksum_entry(const uint8_t* __restrict__ bytes, const SegSrc& src,
                                               const uint32_t* __restrict__ init, uint32_t init_step,
                                               const uint8_t* __restrict__ odd, uint32_t odd_step,
                                               void* __restrict__ out, uint64_t n, uint32_t remap,
                                               const u32x4* __restrict__ zero16) {
  const uint32_t blk = block_order(remap);
  if constexpr (MODE == 3 && NT && UNROLL == 8 && (LPS == 32 || LPS == 64)) {
    // the last bin's launch under kPlanWhole16: every segment of the batch,
    // 16-lane groups in the first n/16 (logical) blocks, the rest exit
    if (src.list && src.bin == kBins - 1 && src.meta[kBinMetaPlan] == kPlanWhole16) {
      constexpr uint32_t kG16 = kBlock / 16;
      const uint64_t need = (n + kG16 - 1) / kG16;
      const uint32_t nblk16 = uint32_t(need < gridDim.x ? need : gridDim.x);
      if (blk >= nblk16) return;
      SegSrc whole = src;
      whole.list = nullptr;  // resolve(): every segment by index
      checksum_body<16, 8, true, 3, OUT>(bytes, whole, init, init_step, odd, odd_step, out, n, blk, nblk16);
      return;
    }
    // ... under kPlanWholeSmall: ACK-sized segments (mean <= kTinyMaxAvg
    // bytes) one per lane in the first n/256 (logical) blocks, otherwise the
    // small-segment body (4 lanes, 2 segments per group in flight) in the
    // first n/128
    if (src.list && src.bin == kBins - 1 && src.meta[kBinMetaPlan] == kPlanWholeSmall &&
        src.meta[kBinMetaAvgLen] <= kTinyMaxAvg) {
      const uint64_t need = (n + kBlock - 1) / kBlock;
      const uint32_t nblks = uint32_t(need < gridDim.x ? need : gridDim.x);
      if (blk >= nblks) return;
      SegSrc whole = src;
      whole.list = nullptr;
      checksum_tiny_body<OUT>(bytes, whole, init, init_step, odd, odd_step, zero16, out, n, blk, nblks);
      return;
    }
    if (src.list && src.bin == kBins - 1 && src.meta[kBinMetaPlan] == kPlanWholeSmall) {
      constexpr uint32_t kPerBlock = (kBlock / 4) * 2;
      const uint64_t need = (n + kPerBlock - 1) / kPerBlock;
      const uint32_t nblks = uint32_t(need < gridDim.x ? need : gridDim.x);
      if (blk >= nblks) return;
      SegSrc whole = src;
      whole.list = nullptr;
      checksum_small_body<4, 2, 2, OUT>(bytes, whole, init, init_step, odd, odd_step, zero16, out, n, blk, nblks);
      return;
    }
  }
  // a bin launch whose bin is empty (the last bin under the split plan) is
  // dispatch-bound — ~0.05 ns per wave whatever the block shape (measured,
  // git 7692616:tools/probe/dispatch_probe.hip) — so its waves leave before anything else
  if (src.list && resolve(src, n).items == 0) return;
  checksum_body<LPS, UNROLL, NT, MODE, OUT>(bytes, src, init, init_step, odd, odd_step, out, n, blk,
                                            gridDim.x);
}

template <int LPS, int UNROLL, bool NT, int MODE, int OUT>
__global__ __launch_bounds__(kBlock) void k_checksum(const uint8_t* __restrict__ bytes, SegSrc src,
                                                     const uint32_t* __restrict__ init,
                                                     uint32_t init_step,
                                                     const uint8_t* __restrict__ odd,
                                                     uint32_t odd_step,
                                                     void* __restrict__ out, uint64_t n, uint32_t remap,
                                                     const u32x4* __restrict__ zero16, Done done) {
  bytes = rebase(bytes, src);
  checksum_entry<LPS, UNROLL, NT, MODE, OUT>(bytes, src, init, init_step, odd, odd_step, out, n, remap, zero16);
  signal_done(done);
}

template <int LPS, int UNROLL, int SEGS, int OUT>
__global__ __launch_bounds__(kBlock) void k_checksum_small(const uint8_t* __restrict__ bytes, SegSrc src,
                                                           const uint32_t* __restrict__ init,
                                                           uint32_t init_step,
                                                           const uint8_t* __restrict__ odd,
                                                           uint32_t odd_step,
                                                           const u32x4* __restrict__ zero16,
                                                           void* __restrict__ out, uint64_t n, Done done) {
  bytes = rebase(bytes, src);
  checksum_small_body<LPS, UNROLL, SEGS, OUT>(bytes, src, init, init_step, odd, odd_step, zero16, out, n,
                                              blockIdx.x, gridDim.x);
  signal_done(done);
}

template <int OUT>
__global__ __launch_bounds__(kBlock) void k_checksum_tiny(const uint8_t* __restrict__ bytes, SegSrc src,
                                                          const uint32_t* __restrict__ init, uint32_t init_step,
                                                          const uint8_t* __restrict__ odd, uint32_t odd_step,
                                                          const u32x4* __restrict__ zero16, void* __restrict__ out,
                                                          uint64_t n, Done done) {
  bytes = rebase(bytes, src);
  checksum_tiny_body<OUT>(bytes, src, init, init_step, odd, odd_step, zero16, out, n, blockIdx.x, gridDim.x);
  signal_done(done);
}

// Two-class launch for receive mixes (ACKs among MTU segments), no binning
// pass: block b takes segments [4 SPW b, 4 SPW b + 4 SPW); wave w reads the
// bounds of SPW of them and appends each to the block's short (<= 4 chunks)
// or long list in LDS.  Wave 0 then finishes the short ones one per lane (64
// per pass, as k_checksum_tiny does), while every wave — wave 0 once its
// short passes are done — claims the long ones 64 / LONG_LPS at a time from
// an LDS counter (LONG_LPS lanes each, the line grid, unroll 8).  The fused
// IPv4 launch's block lists (k_ipv4_twoclass); 2 M x 40 / 1460 B 230.8 ->
// 224.8 us against the per-wave version (git 7692616:tools/probe/csum_mix_probe.hip).
template <int LONG_LPS, int SPW, int OUT>
__global__ __launch_bounds__(kBlock) void k_checksum_twoclass(const uint8_t* __restrict__ bytes, SegSrc src,
                                                              const uint32_t* __restrict__ init, uint32_t init_step,
                                                              const uint8_t* __restrict__ odd, uint32_t odd_step,
                                                              const u32x4* __restrict__ zero16,
                                                              void* __restrict__ out, uint64_t n, uint32_t remap) {
  constexpr uint32_t kPer = (kBlock / 64) * SPW;
  __shared__ uint64_t lst[kPer][2], sst[kPer][2];  // the block's long / short segments' {start, end}
  __shared__ uint32_t lseg[kPer], sseg[kPer];
  __shared__ uint32_t cnt[3];  // long, short, long claimed
  __shared__ uint32_t o_sum[kPer];  // the block's sums, written out as one coalesced row at the end
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  bytes = rebase(bytes, src);
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  const Work w{n, nullptr};
  const uint64_t bb = uint64_t(block_order(remap)) * kPer;  // the block's segments [bb, bb + kPer) (no list)
  const uint64_t gi = bb + wv * SPW + (lane < SPW ? lane : 0u);
  uint64_t seg, s, e;
  src_locate(src, w, gi, n, seg, s, e);
  const bool valid = gi < n && lane < SPW;
  const uint64_t a0 = s & ~uint64_t(15);
  const uint32_t nch = uint32_t(((e > s ? e - a0 : 0) + 15) >> 4);
  const bool is_short = nch <= 4;
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
    lseg[lbase + lr] = uint32_t(seg);
  }
  if (valid && is_short) {
    sst[sbase + sr][0] = s;
    sst[sbase + sr][1] = e;
    sseg[sbase + sr] = uint32_t(seg);
  }
  __syncthreads();
  const uint32_t nlong = cnt[0], nshort = cnt[1];
  auto store = [&](uint64_t sg, uint32_t sum) { o_sum[sg - bb] = sum; };
  if (wv == 0)
    for (uint32_t r0 = 0; r0 < nshort; r0 += 64) {  // uniform
      const uint32_t k = r0 + lane;
      const bool mine = k < nshort;
      const uint32_t kc = mine ? k : 0u;
      const uint64_t ss = sst[kc][0], se = mine ? sst[kc][1] : ss;
      const uint64_t sg = sseg[kc];
      const uint64_t b0 = ss & ~uint64_t(15), span = se > ss ? se - b0 : 0;
      const uint32_t nc = uint32_t((span + 15) >> 4);
      const u32x4* __restrict__ p = reinterpret_cast<const u32x4*>(bytes + b0);
      u32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // an empty slot loads the zero block
        const u32x4* q = nc ? p + (uint32_t(u) < nc ? uint32_t(u) : nc - 1) : zero16;
        if (nc) ICS_CHECK16(q, bytes + b0, bytes + b0 + (uint64_t(nc) << 4));
        v[u] = *q;
      }
      const uint32_t i0 = init[sg * init_step];
      const uint32_t sw = (uint32_t(ss) ^ uint32_t(odd[sg * odd_step])) & 1u;
      uint32_t ev = 0, od = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint64_t at = uint64_t(u) << 4;
        const uint32_t lo = u == 0 ? uint32_t(ss) & 15u : 0u;
        const uint32_t hi = at >= span ? 0u : (span - at >= 16 ? 16u : uint32_t(span - at));
        acc_chunk(v[u] & byte_range_mask(lo, hi), ev, od);
      }
      if (mine) store(sg, i0 + combine_roles(ev, od, sw));
    }
  constexpr uint32_t kGroups = 64 / LONG_LPS;
  const uint32_t g = lane / LONG_LPS, gl = lane & (LONG_LPS - 1);
  for (;;) {
    uint32_t r0 = 0;
    if (lane == 0) r0 = atomicAdd(&cnt[2], kGroups);
    r0 = __builtin_amdgcn_readfirstlane(r0);
    if (r0 >= nlong) break;  // uniform
    const uint32_t k = r0 + g;
    const bool mine = k < nlong;
    const uint32_t kc = mine ? k : 0u;
    const uint64_t ls = mine ? lst[kc][0] : 0, le = mine ? lst[kc][1] : 0;
    const uint64_t lsg = lseg[kc];
    const uint32_t i0 = init[lsg * init_step];
    const uint32_t sw = (uint32_t(ls) ^ uint32_t(odd[lsg * odd_step])) & 1u;
    uint32_t ev = 0, od = 0;
    // 7 loads per lane: an MSS segment's line-grid span (<= 100 chunks) in one
    // pass of 112 chunks, fewer clamped slot loads than 8 (2 M bimodal
    // 226.6 -> 221.1 us, profiles/r4_ab_csum_twoclass_unroll7.jsonl)
    range_sums_line_primed<LONG_LPS, 7, true>(bytes, ls, le, gl, ev, od);
    const uint32_t tot = group_sum<LONG_LPS>(combine_roles(ev, od, sw));
    if (mine && gl == LONG_LPS - 1) store(lsg, i0 + tot);
  }
  __syncthreads();
  const uint64_t i = bb + threadIdx.x;  // every segment of the block was summed: its row is complete
  if (threadIdx.x < kPer && i < n) {
    if (OUT == 0)
      static_cast<uint16_t*>(out)[i] = fold_value(o_sum[threadIdx.x]);
    else
      static_cast<uint32_t*>(out)[i] = o_sum[threadIdx.x];
  }
}

// Dense fixed-stride batches of short segments (stride == seg_len == 16*LPS,
// 16-byte aligned base — config 3's 1 M x 64 B TCP segments): the batch is one
// flat array of 16-byte chunks, every chunk belongs whole to one segment, so
// a wave instruction reads 1 KiB contiguous and no slot needs a mask, an
// address clamp or a boundary case.  Lane group g of wave w owns segments
// (w*SEGS + k)*kSegsPerWave + g, k < SEGS: all SEGS loads (plus the init
// words) are issued before the first is consumed.  Every start is even (the
// base is aligned, the stride a multiple of 16), so byte roles never swap.
// Measured floor for 64 MiB + 4 MiB inits + 2 MiB outputs on MI355X:
// ≈12.4 us (git 7692616:tools/probe/small_probe.hip).
// (block blk of the launch; init_step 0 reads one shared zero word)
template <int LPS, int SEGS, bool INIT, int OUT>
__device__ __forceinline__ void checksum_dense_body(const u32x4* __restrict__ chunks, const uint32_t* __restrict__ init,
                                                    uint32_t init_step, void* __restrict__ out, uint64_t n,
                                                    uint32_t blk) {
  constexpr uint32_t kSegsPerWave = 64 / LPS;
  const uint32_t lane64 = threadIdx.x & 63u, lane = threadIdx.x & (LPS - 1), group = lane64 / LPS;
  const uint64_t wave = (uint64_t(blk) * kBlock + threadIdx.x) >> 6;
  const uint64_t seg0 = wave * SEGS * kSegsPerWave + group;
  const uint64_t nch = n * LPS;
  u32x4 v[SEGS];
  uint32_t i0[SEGS];
#pragma unroll
  for (int k = 0; k < SEGS; ++k) {
    const uint64_t seg = seg0 + uint64_t(k) * kSegsPerWave;
    const uint64_t c = seg * LPS + lane;
    ICS_CHECK16(chunks + (c < nch ? c : nch - 1), reinterpret_cast<const uint8_t*>(chunks),
                reinterpret_cast<const uint8_t*>(chunks + nch));
    v[k] = __builtin_nontemporal_load(chunks + (c < nch ? c : nch - 1));
    i0[k] = INIT ? init[(seg < n ? seg : n - 1) * init_step] : 0u;
  }
#pragma unroll
  for (int k = 0; k < SEGS; ++k) {
    uint32_t ev = 0, od = 0;
    acc_chunk(v[k], ev, od);
    const uint32_t tot = group_sum<LPS>(ev * 256u + od);
    const uint64_t seg = seg0 + uint64_t(k) * kSegsPerWave;
    if (seg < n && lane == LPS - 1) {
      const uint32_t sum = i0[k] + tot;
      if (OUT == 0)
        static_cast<uint16_t*>(out)[seg] = fold_value(sum);
      else
        static_cast<uint32_t*>(out)[seg] = sum;
    }
  }
}

template <int LPS, int SEGS, bool INIT, int OUT>
__global__ __launch_bounds__(kBlock) void k_checksum_dense(const u32x4* __restrict__ chunks,
                                                           const uint32_t* __restrict__ init,
                                                           void* __restrict__ out, uint64_t n) {
  checksum_dense_body<LPS, SEGS, INIT, OUT>(chunks, init, 1u, out, n, blockIdx.x);
}

// Bins 0..kBins-2 of a binned batch in ONE launch: nblk blocks per bin, each
// bin with its own geometry (kBinGeometry; blocks of bin b = [b*nblk,
// (b+1)*nblk)).  One launch instead of four: no drain between bins, and one
// launch to skip under the whole-batch plan.
template <int OUT>
__global__ __launch_bounds__(kBlock) void k_checksum_bins(const uint8_t* __restrict__ bytes, SegSrc src,
                                                          const uint32_t* __restrict__ init, uint32_t init_step,
                                                          const uint8_t* __restrict__ odd, uint32_t odd_step,
                                                          const u32x4* __restrict__ zero16,
                                                          void* __restrict__ out, uint64_t n, uint32_t nblk) {
  const uint32_t b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
  bytes = rebase(bytes, src);
  SegSrc bs = src;
  bs.list = src.list + uint64_t(b) * n;
  bs.bin = int(b);
  static_assert(bin_geometry_is(0, 4, 2, 2, 2) && bin_geometry_is(1, 16, 4, 3, 1) && bin_geometry_is(2, 16, 8, 3, 1) &&
                    bin_geometry_is(3, 32, 4, 3, 1), "the bodies below are kBinGeometry's (what bin_geometry reports)");
  switch (b) {
    case 0:
      checksum_small_body<4, 2, 2, OUT>(bytes, bs, init, init_step, odd, odd_step, zero16, out, n, blk, nblk);
      break;
    case 1:
      checksum_body<16, 4, true, 3, OUT>(bytes, bs, init, init_step, odd, odd_step, out, n, blk, nblk);
      break;
    case 2:
      checksum_body<16, 8, true, 3, OUT>(bytes, bs, init, init_step, odd, odd_step, out, n, blk, nblk);
      break;
    default:
      checksum_body<32, 4, true, 3, OUT>(bytes, bs, init, init_step, odd, odd_step, out, n, blk, nblk);
      break;
  }
}

__global__ void k_fold(const uint32_t* __restrict__ sum, uint16_t* __restrict__ out, uint64_t n) {
  ICS_GRID_STRIDE(i, n) out[i] = fold_value(sum[i]);
}

template <int LPS, int UNROLL, bool NT, int MODE>
hipError_t launch_checksum_t(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out,
                             int out_kind, uint32_t max_blocks, hipStream_t st) {
  const uint32_t blocks = blocks_for(sp.n, kBlock / LPS, max_blocks);
  const SegWords w = seg_words(init, odd, sp.zero16);
  with_out(out_kind, [&](auto OUT) {
    hipLaunchKernelGGL((k_checksum<LPS, UNROLL, NT, MODE, OUT()>), dim3(blocks), dim3(kBlock), 0, st, sp.bytes,
                       src_of(sp), w.ip, w.is, w.op, w.os, out, sp.n, g_xcd_remap,
                       static_cast<const u32x4*>(sp.zero16), sp.done);
  });
  return hipGetLastError();
}

template <int LPS, int UNROLL, int SEGS>
hipError_t launch_checksum_small_t(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out,
                                   int out_kind, uint32_t max_blocks, hipStream_t st) {
  const uint32_t blocks = blocks_for((sp.n + SEGS - 1) / SEGS, kBlock / LPS, max_blocks);
  const SegWords w = seg_words(init, odd, sp.zero16);
  const u32x4* z = static_cast<const u32x4*>(sp.zero16);
  with_out(out_kind, [&](auto OUT) {
    hipLaunchKernelGGL((k_checksum_small<LPS, UNROLL, SEGS, OUT()>), dim3(blocks), dim3(kBlock), 0, st, sp.bytes,
                       src_of(sp), w.ip, w.is, w.op, w.os, z, out, sp.n, sp.done);
  });
  return hipGetLastError();
}

template <int LONG_LPS, int SPW>
hipError_t launch_twoclass_t(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out, int out_kind,
                             uint32_t remap, uint32_t lds_pad, hipStream_t st) {
  const uint64_t blocks = twoclass_blocks(sp.n, SPW);
  if (blocks == 0 || blocks > kMaxGridBlocks) return hipErrorInvalidValue;
  const SegWords w = seg_words(init, odd, sp.zero16);
  const u32x4* z = static_cast<const u32x4*>(sp.zero16);
  with_out(out_kind, [&](auto OUT) {
    hipLaunchKernelGGL((k_checksum_twoclass<LONG_LPS, SPW, OUT()>), dim3(uint32_t(blocks)), dim3(kBlock), lds_pad,
                       st, sp.bytes, src_of(sp), w.ip, w.is, w.op, w.os, z, out, sp.n, remap);
  });
  return hipGetLastError();
}

hipError_t launch_checksum_tiny_t(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out,
                                  int out_kind, uint32_t max_blocks, hipStream_t st) {
  const uint32_t blocks = blocks_for(sp.n, kBlock, max_blocks);
  const SegWords w = seg_words(init, odd, sp.zero16);
  const u32x4* z = static_cast<const u32x4*>(sp.zero16);
  with_out(out_kind, [&](auto OUT) {
    hipLaunchKernelGGL(k_checksum_tiny<OUT()>, dim3(blocks), dim3(kBlock), 0, st, sp.bytes, src_of(sp), w.ip, w.is,
                       w.op, w.os, z, out, sp.n, sp.done);
  });
  return hipGetLastError();
}

template <int LPS, int SEGS>
hipError_t launch_dense_t(const SegSpec& sp, const uint32_t* init, void* out, int out_kind, hipStream_t st) {
  const uint64_t segs_per_block = uint64_t(kBlock / LPS) * SEGS;
  const uint64_t blocks = (sp.n + segs_per_block - 1) / segs_per_block;
  if (blocks == 0 || blocks > (uint64_t(1) << 22)) return hipErrorInvalidValue;
  const u32x4* c = reinterpret_cast<const u32x4*>(sp.bytes);
  with_flag(init != nullptr, [&](auto INIT) {
    with_out(out_kind, [&](auto OUT) {
      hipLaunchKernelGGL((k_checksum_dense<LPS, SEGS, INIT(), OUT()>), dim3(uint32_t(blocks)), dim3(kBlock), 0, st, c,
                         init, out, sp.n);
    });
  });
  return hipGetLastError();
}

}  // namespace

// Geometry choice from the (average) segment length, measured on MI355X
// (git 7692616:tools/sweep_geometry.py; profiles/r1_sweep_geometry.jsonl,
// r1_sweep_line_grid.jsonl, r1_sweep_small.jsonl).  Small segments
// (<= ~270 B): k_checksum_small with about one load slot per 16-byte chunk
// and 2 segments per lane group in flight (64 B = 4 lanes x 1 load x 2).
// From ~270 bytes up: the 128-byte-line grid with default-policy boundary
// loads first (mode 3, range_sums_line_primed; profiles/r1_sweep_primed.jsonl)
// with slots >= chunks + 8 so one step covers a segment (1500 B -> 16 lanes x
// 8 loads), and 64 x 8 (8 KiB per wave step) looping for long segments.
// Interior chunks stream non-temporally (read once).
//
// Round 2 (git 7692616:tools/sweep_geometry.py, profiles/r2_sweep_mtu.jsonl,
// r2_sweep_mid.jsonl; 1 M segments, GB/s of the best vs the round-1 pick):
// slots close above the chunks a line-anchored segment spans win — 1000 B
// (16,5) 7569 vs (16,8) 6577, 1040 B (16,5) 7526 vs 6394, 1200 B (16,6) 7571
// vs 7133, 2000 B (16,4) 7477 vs (32,4) 7107, 2500 B (32,8) 7486 vs 7359,
// 3000 B (32,8) 7416 vs 7294, 4096 B (64,8) 7561 vs 7324; 600/800 B keep
// (16,4), 1460/1500 B (16,8).
Geometry pick_geometry(uint64_t avg_len) {
  const uint64_t m = (avg_len + 15) / 16;  // 16-byte chunks of the payload
  if (avg_len <= kTinyMaxAvg) return {1, 4, false, kModeTiny, 1};  // one lane per segment (ACK-sized)
  if (m <= 5) return {4, 1, true, 2, 2};   // small-segment kernel, 2 segments per group in flight
  if (m <= 9) return {4, 2, true, 2, 2};
  if (m <= 17) return {8, 2, true, 2, 2};
  if (m <= 56) return {16, 4, true, 3, 1};
  if (m <= 69) return {16, 5, true, 3, 1};
  if (m <= 82) return {16, 6, true, 3, 1};
  if (m <= 120) return {16, 8, true, 3, 1};
  if (m <= 140) return {16, 4, true, 3, 1};
  if (m <= 220) return {32, 8, true, 3, 1};
  return {64, 8, true, 3, 1};
}

hipError_t launch_checksum(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out,
                           int out_kind, Geometry g, uint32_t max_blocks, hipStream_t st) {
  if (g.mode == kModeTiny) return launch_checksum_tiny_t(sp, init, odd, out, out_kind, max_blocks, st);
  hipError_t e = hipErrorInvalidValue;  // no such geometry
  if (g.segs > 1)
    for_small_geometry(g, [&](auto L, auto U, auto K) {
      e = launch_checksum_small_t<L(), U(), K()>(sp, init, odd, out, out_kind, max_blocks, st);
    });
  else
    for_geometry(g, [&](auto L, auto U, auto T, auto A) {
      e = launch_checksum_t<L(), U(), T(), A()>(sp, init, odd, out, out_kind, max_blocks, st);
    });
  return e;
}

hipError_t launch_checksum_twoclass(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out,
                                    int out_kind, int spw, uint32_t remap, hipStream_t st, uint32_t lds_pad) {
  if (sp.list) return hipErrorInvalidValue;
  if (spw == 32) return launch_twoclass_t<16, 32>(sp, init, odd, out, out_kind, remap, lds_pad, st);
  if (spw == 16) return launch_twoclass_t<16, 16>(sp, init, odd, out, out_kind, remap, lds_pad, st);
  if (spw == 8) return launch_twoclass_t<16, 8>(sp, init, odd, out, out_kind, remap, lds_pad, st);
  return hipErrorInvalidValue;
}

bool dense_supported(const SegSpec& sp) {
  if (sp.offsets || sp.n == 0 || sp.stride != sp.seg_len) return false;
  if ((reinterpret_cast<uintptr_t>(sp.bytes) & 15) != 0) return false;
  return sp.seg_len == 32 || sp.seg_len == 64 || sp.seg_len == 128;
}

hipError_t launch_checksum_dense(const SegSpec& sp, const uint32_t* init, void* out, int out_kind, int segs,
                                 hipStream_t st) {
  if (!dense_supported(sp)) return hipErrorInvalidValue;
  const int lps = int(sp.seg_len / 16);
#define ICS_DENSE_CASE(L, K) \
  if (lps == L && segs == K) return launch_dense_t<L, K>(sp, init, out, out_kind, st);
  ICS_DENSE_CASE(2, 2) ICS_DENSE_CASE(2, 4) ICS_DENSE_CASE(2, 8)
  ICS_DENSE_CASE(4, 1) ICS_DENSE_CASE(4, 2) ICS_DENSE_CASE(4, 4) ICS_DENSE_CASE(4, 8)
  ICS_DENSE_CASE(8, 1) ICS_DENSE_CASE(8, 2) ICS_DENSE_CASE(8, 4)
#undef ICS_DENSE_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_checksum_bins(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out,
                                int out_kind, uint32_t blocks_per_bin, hipStream_t st) {
  if (!sp.list || blocks_per_bin == 0) return hipErrorInvalidValue;
  if (blocks_per_bin > (1u << 20)) blocks_per_bin = 1u << 20;  // grid work-items stay < 2^32
  const SegWords w = seg_words(init, odd, sp.zero16);
  const u32x4* z = static_cast<const u32x4*>(sp.zero16);
  const dim3 grid(blocks_per_bin * (kBins - 1));
  with_out(out_kind, [&](auto OUT) {
    hipLaunchKernelGGL(k_checksum_bins<OUT()>, grid, dim3(kBlock), 0, st, sp.bytes, src_of(sp), w.ip, w.is, w.op,
                       w.os, z, out, sp.n, blocks_per_bin);
  });
  return hipGetLastError();
}

bool geometry_supported(Geometry g) {
  if (g.mode == kModeTiny) return g.lps == 1 && g.segs == 1;
  const auto matched = [](auto...) {};  // supported: the chain launch_checksum walks finds it
  return g.segs > 1 ? for_small_geometry(g, matched) : for_geometry(g, matched);
}

hipError_t launch_fold(const uint32_t* sum, uint16_t* out, uint64_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_fold, dim3(ew_blocks(n)), dim3(kBlock), 0, st, sum, out, n);
  return hipGetLastError();
}

}  // namespace icsum
