// icsum_binning.h — length binning of an offsets batch: the stats, plan and
// scatter passes (k_bin_stats, k_bin_plan, k_bin_scatter) and their launchers.
#pragma once

#include "icsum_common.h"

namespace icsum {
namespace {

// ------------------------------------------------------- length binning ---
// Bin of a segment by its 16-byte chunk count; the boundaries are those of
// pick_geometry, so bin b runs with the geometry pick_geometry gives a batch
// of such segments.
constexpr uint64_t kBinMaxChunks[kBins - 1] = {9, 56, 120, 256};
constexpr int kBinPerThread = 8;  // segments per thread per tile
constexpr int kBinTile = kBlock * kBinPerThread;
constexpr int kBinField = 12;  // bits per bin in a packed count

__device__ __forceinline__ int bin_of(uint64_t len) {
  const uint64_t m = (len + 15) >> 4;
  int b = 0;
#pragma unroll
  for (int k = 0; k < kBins - 1; ++k) b += m > kBinMaxChunks[k];
  return b;
}

// Packed per-bin counts: kBins fields of 12 bits in a uint64 (a tile holds
// 2048 segments, so no field overflows and adding packed words never carries
// across fields).
__device__ __forceinline__ uint32_t field(uint64_t p, int b) {
  return uint32_t(p >> (kBinField * b)) & ((1u << kBinField) - 1);
}

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t u = __shfl_up(v, d, 64);
    if (lane >= uint32_t(d)) v += u;
  }
  return v;
}

// exclusive block scan of packed counts; returns the block total in `total`
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t& total) {
  __shared__ uint64_t wsum[kBlock / 64];
  const uint64_t inc = wave_incl_scan(v);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wsum[w] = inc;
  __syncthreads();
  uint64_t before = 0;
  total = 0;
#pragma unroll
  for (uint32_t k = 0; k < kBlock / 64; ++k) {
    before += k < w ? wsum[k] : 0;
    total += wsum[k];
  }
  __syncthreads();  // wsum is reused by the next tile
  return before + inc - v;
}

// Dispatch plan of a binned batch, decided on the device (k_bin_plan, one
// block after the stats pass) from
// the bin sizes the binning pass recorded, with no host round trip:
//   kPlanWhole  the last bin's launch takes every segment with its own
//               (64- or 32-lane) geometry; the other launches exit at once
//   kPlanSplit  every bin runs from its list with its own geometry
//   kPlanWhole16 the last bin's launch takes every segment with 16-lane
//               groups in its first n/16 blocks (the rest exit at once)
//   kPlanWholeSmall the last bin's launch takes every segment through the
//               small-segment body (or one lane per segment for ACK-sized means)
// The choice is the cheapest plan under kPlanCost (below): every estimate is
// in ns, a sum over the bins of max(bytes / rate, segments * per-segment
// cost) plus the dispatch of the last bin's idle waves.
// Measured under each forced plan (git 7692616:tools/ab_lastbin.py --var ICSUM_BIN_PLAN,
// profiles/r1_ab_plans.jsonl), µs whole / split / whole16: config 4
// 1429 / 1622 / 1682, 2 M bimodal 40+1460 B 525 / 473 / 364, 2 M x 4-6 KiB
// 1515 / 1589 / 1593, 1 M x 1460 B 520 / 429 / 296, 1 M x 40 B 451 / 168 / 205.
struct PlanCostTable {
  // rates in GB/s (= bytes per ns), per-segment costs in ns x 100; sources in profiles/
  uint32_t whole_rate;            // whole: 64-lane groups over a long mix; config 4 whole 1429 us = 7.2 TB/s (r1_ab_plans)
  uint32_t whole_seg_c;           // whole: ns x 100 per segment floor; 1 M x 40 B whole 451 us (r1_ab_plans)
  uint32_t split_fixed_ns;        // split: the scatter pass and the bins 0-3 launch, 26 us fixed (git 7692616:tools/ab_bins.py, r1_ab_bins)
  uint32_t empty_wave_ps;         // every plan: an idle wave of the last bin's launch, 0.053 ns (git 7692616:tools/probe/dispatch_probe.hip)
  uint32_t split_rate_bins;       // split: bins 0-3 from their lists, 5.0 TB/s (r1_ab_bins)
  uint32_t split_rate_last;       // split: last bin, segments no longer contiguous, 6.4 TB/s (r1_ab_bins)
  uint32_t split_seg_c;           // split: ns x 100 per listed segment (r1_ab_bins: 1 M x 40 B split 168 us)
  uint32_t w16_rate[kBins];       // whole16 per bin: 7.0 TB/s to 1920 B, 6.5 to 4 KiB, 5.0 above (16 lanes loop; r1_ab_plans)
  uint32_t w16_seg_c;             // whole16: ns x 100 per segment (1 M x 1460 B whole16 296 us)
  uint32_t small_rate[kBins];     // wholeS per bin: 5.0 TB/s for bin 0, 0.8 for longer (4 lanes loop; r1_ab_plans small)
  uint32_t small_seg_c[kBins];    // wholeS: ns x 100 per segment, 0.02 bin 0 / 0.5 longer (1 M x 40-43 B small 140 us)
};
constexpr PlanCostTable kPlanCost = {7100, 45, 26000, 53, 5000, 6400, 10,
                                     {7000, 7000, 7000, 6500, 5000}, 16,
                                     {5000, 800, 800, 800, 800}, {2, 50, 50, 50, 50}};

__global__ __launch_bounds__(kBlock) void k_bin_plan(uint32_t* __restrict__ meta, const uint32_t* __restrict__ cnt_part,
                                                     const uint64_t* __restrict__ by_part, uint32_t parts, uint64_t n,
                                                     int force, uint32_t last_lps, uint64_t* __restrict__ plan_out,
                                                     uint32_t gen) {
  // totals per bin from the stats pass's per-block partials (parts <= kBlock:
  // one partial per thread, all loads in flight together)
  __shared__ uint32_t wc[kBlock / 64][kBins];
  __shared__ uint64_t wb[kBlock / 64][kBins];
  const uint32_t w = threadIdx.x >> 6;
  const bool mine = threadIdx.x < parts;
  uint32_t cs[kBins];
  uint64_t vs[kBins];
#pragma unroll
  for (int k = 0; k < kBins; ++k) {
    cs[k] = mine ? cnt_part[k * parts + threadIdx.x] : 0;
    vs[k] = mine ? by_part[k * parts + threadIdx.x] : 0;
  }
#pragma unroll
  for (int k = 0; k < kBins; ++k) {
    uint32_t c = cs[k];
    uint64_t v = vs[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      c += __shfl_xor(c, d, 64);
      v += __shfl_xor(v, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      wc[w][k] = c;
      wb[w][k] = v;
    }
  }
  // the scatter pass's cursors start at 0 (zeroed here, in stream order before
  // it, instead of by a separate memset launch: one dispatch less per batch)
  if (threadIdx.x < kBins) meta[kBinMetaCursor + threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint64_t waves = n * last_lps / 64;  // the last bin's launch
    const PlanCostTable& C = kPlanCost;
    uint64_t total = 0, short_n = 0, long_bytes = 0;
    uint64_t t_split = C.split_fixed_ns + waves * C.empty_wave_ps / 1000;
    uint64_t t16 = (waves - n / 4) * C.empty_wave_ps / 1000;        // whole16 uses the first n/16 blocks
    uint64_t t_small = (waves - n / 32) * C.empty_wave_ps / 1000;   // wholeS the first n/128
#pragma unroll
    for (int k = 0; k < kBins; ++k) {
      uint32_t c = 0;
      uint64_t v = 0;
#pragma unroll
      for (uint32_t q = 0; q < kBlock / 64; ++q) {
        c += wc[q][k];
        v += wb[q][k];
      }
      meta[kBinMetaCount + k] = c;
      if (k == 0) short_n = c;
      if (k >= 3) long_bytes += v;  // segments > 1920 bytes
      total += v;
      const uint64_t tb = v / (k == kBins - 1 ? C.split_rate_last : C.split_rate_bins), tn = uint64_t(c) * C.split_seg_c / 100;
      t_split += tb > tn ? tb : tn;
      const uint64_t sb = v / C.w16_rate[k], sn = uint64_t(c) * C.w16_seg_c / 100;
      t16 += sb > sn ? sb : sn;
      const uint64_t mb = v / C.small_rate[k], mn = uint64_t(c) * C.small_seg_c[k] / 100;
      t_small += mb > mn ? mb : mn;
    }
    const uint64_t tb = total / C.whole_rate, tn = n * C.whole_seg_c / 100, t_whole = tb > tn ? tb : tn;
    uint32_t plan = kPlanWhole;
    if (force >= 0) {
      plan = uint32_t(force);
    } else {
      uint64_t best = t_whole;
      if (t_split < best) best = t_split, plan = kPlanSplit;
      if (t16 < best) best = t16, plan = kPlanWhole16;
      if (t_small < best) plan = kPlanWholeSmall;
    }
    meta[kBinMetaPlan] = plan;
    const uint64_t avg = n ? total / n : 0;
    meta[kBinMetaAvgLen] = uint32_t(avg < 0xFFFFFFFFull ? avg : 0xFFFFFFFFull);
    // the host's plan cache (icsum_dispatch.cpp), one 8-byte store to page-locked
    // host memory: the plan (bits 0-3), the share of bin-0 (<= 144-byte)
    // segments in sixteenths (bits 4-7), the batch size (bits 8-39), the
    // share of bytes in segments over 1920 bytes in sixteenths (bits 40-43)
    // the mean segment length in bytes, capped at 4095 (bits 44-55), and the
    // generation of the cache slot that asked for it (bits 56-63)
    const uint64_t short16 = n ? short_n * 16 / n : 0, long16 = total ? long_bytes * 16 / total : 0;
    if (plan_out)
      *plan_out = plan | ((short16 < 15 ? short16 : 15) << 4) | ((n & 0xFFFFFFFFull) << 8) |
                  ((long16 < 15 ? long16 : 15) << 40) | ((avg < 4095 ? avg : 4095) << 44) |
                  (uint64_t(gen & 0xffu) << 56);
  }
}

// Pass 1: segments and bytes per bin, one partial per block (no same-address
// atomics: they serialise at a few ns each; no last-block reduction: its
// device-wide fence writes back L2 in every block); k_bin_plan adds them up.
__global__ __launch_bounds__(kBlock) void k_bin_stats(const uint64_t* __restrict__ off, uint64_t n,
                                                      uint32_t* __restrict__ cnt_part,
                                                      uint64_t* __restrict__ by_part) {
  uint32_t cnt[kBins] = {};
  uint64_t by[kBins] = {};
  // tiles of kBinTile segments; a thread's kBinPerThread offset pairs are all
  // requested before any is used
  for (uint64_t t0 = uint64_t(blockIdx.x) * kBinTile; t0 < n; t0 += uint64_t(gridDim.x) * kBinTile) {
    uint64_t a[kBinPerThread], z[kBinPerThread];
#pragma unroll
    for (int j = 0; j < kBinPerThread; ++j) {
      const uint64_t i = t0 + uint64_t(j) * kBlock + threadIdx.x;
      const uint64_t c = i < n ? i : n - 1;
      a[j] = off[c];
      z[j] = off[c + 1];
    }
#pragma unroll
    for (int j = 0; j < kBinPerThread; ++j) {
      const bool in = t0 + uint64_t(j) * kBlock + threadIdx.x < n;
      const uint64_t len = z[j] - a[j];
      const int b = bin_of(len);
#pragma unroll
      for (int k = 0; k < kBins; ++k) {
        cnt[k] += in && b == k;
        by[k] += in && b == k ? len : 0;
      }
    }
  }
  __shared__ uint32_t wc[kBlock / 64][kBins];
  __shared__ uint64_t wb[kBlock / 64][kBins];
  const uint32_t w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kBins; ++k) {
    uint32_t c = cnt[k];
    uint64_t v = by[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      c += __shfl_xor(c, d, 64);
      v += __shfl_xor(v, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      wc[w][k] = c;
      wb[w][k] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < kBins) {
    uint32_t c = 0;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t q = 0; q < kBlock / 64; ++q) {
      c += wc[q][threadIdx.x];
      v += wb[q][threadIdx.x];
    }
    cnt_part[threadIdx.x * gridDim.x + blockIdx.x] = c;
    by_part[threadIdx.x * gridDim.x + blockIdx.x] = v;
  }
}

// Pass 3 (split plan only): every tile reserves its slice of each bin with
// one atomic per bin (bin b's list holds its entries at list + b * n).
__global__ __launch_bounds__(kBlock) void k_bin_scatter(const uint64_t* __restrict__ off, uint64_t n,
                                                        uint32_t* __restrict__ meta,
                                                        u32x4* __restrict__ list) {
  if (meta[kBinMetaPlan] != kPlanSplit) return;  // whole-batch plans: no lists
  __shared__ uint32_t resv[kBins];
  for (uint64_t t0 = uint64_t(blockIdx.x) * kBinTile; t0 < n; t0 += uint64_t(gridDim.x) * kBinTile) {
    uint64_t s[kBinPerThread], len[kBinPerThread];
    int bin[kBinPerThread];
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < kBinPerThread; ++j) {
      const uint64_t i = t0 + uint64_t(j) * kBlock + threadIdx.x;
      bin[j] = -1;
      if (i < n) {
        s[j] = off[i];
        len[j] = off[i + 1] - s[j];
        bin[j] = bin_of(len[j]);
        mine += uint64_t(1) << (kBinField * bin[j]);
      }
    }
    uint64_t total;
    uint64_t excl = block_excl_scan(mine, total);
    if (threadIdx.x < kBins) {
      const uint32_t c = field(total, threadIdx.x);
      resv[threadIdx.x] = c ? atomicAdd(&meta[kBinMetaCursor + threadIdx.x], c) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kBinPerThread; ++j) {
      if (bin[j] < 0) continue;
      const int b = bin[j];
      const uint64_t pos = uint64_t(b) * n + resv[b] + field(excl, b);
      excl += uint64_t(1) << (kBinField * b);
      const uint64_t i = t0 + uint64_t(j) * kBlock + threadIdx.x;
      const uint32_t l = len[j] < kLongEntry ? uint32_t(len[j]) : kLongEntry;
      list[pos] = u32x4{uint32_t(s[j]), uint32_t(s[j] >> 32), l, uint32_t(i)};
    }
    __syncthreads();  // resv is reused by the next tile
  }
}

// the stats and plan passes (force_plan -1: the device plan decides)
hipError_t bin_stats_plan(const uint64_t* offsets, uint64_t n, uint32_t* meta, int force_plan, uint32_t last_lps,
                          uint64_t* plan_out, uint32_t gen, hipStream_t st) {
  if (!offsets || n == 0 || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
  uint32_t* cnt_part = meta + kBinMetaWords;
  uint64_t* by_part = reinterpret_cast<uint64_t*>(cnt_part + kBins * kBinStatBlocks);
  const uint64_t tiles = (n + kBinTile - 1) / kBinTile;
  const uint32_t parts = uint32_t(tiles < kBinStatBlocks ? tiles : kBinStatBlocks);
  hipLaunchKernelGGL(k_bin_stats, dim3(parts), dim3(kBlock), 0, st, offsets, n, cnt_part, by_part);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(k_bin_plan, dim3(1), dim3(kBlock), 0, st, meta, cnt_part, by_part, parts, n, force_plan,
                     last_lps, plan_out, gen);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_bin_segments(const uint64_t* offsets, uint64_t n, void* list, uint32_t* meta, int force_plan,
                               uint32_t last_lps, uint64_t* plan_out, uint32_t gen, hipStream_t st) {
  if (hipError_t e = bin_stats_plan(offsets, n, meta, force_plan, last_lps, plan_out, gen, st)) return e;
  const uint64_t tiles = (n + kBinTile - 1) / kBinTile;
  hipLaunchKernelGGL(k_bin_scatter, dim3(uint32_t(tiles < 2048 ? tiles : 2048)), dim3(kBlock), 0, st,
                     offsets, n, meta, static_cast<u32x4*>(list));
  return hipGetLastError();
}

hipError_t launch_bin_plan(const uint64_t* offsets, uint64_t n, uint32_t* meta, uint32_t last_lps,
                           uint64_t* plan_out, uint32_t gen, hipStream_t st) {
  return bin_stats_plan(offsets, n, meta, -1, last_lps, plan_out, gen, st);
}

// geometries k_checksum_bins hard-codes for bins 0..kBins-2
constexpr Geometry kBinGeometry[kBins - 1] = {{4, 2, true, 2, 2}, {16, 4, true, 3, 1}, {16, 8, true, 3, 1},
                                              {32, 4, true, 3, 1}};
constexpr bool bin_geometry_is(int b, int lps, int unroll, int mode, int segs) {  // k_checksum_bins' static_assert
  return kBinGeometry[b].lps == lps && kBinGeometry[b].unroll == unroll && kBinGeometry[b].nt &&
         kBinGeometry[b].mode == mode && kBinGeometry[b].segs == segs;
}

Geometry bin_geometry(int bin) {
  // bins 0..kBins-2: the geometries k_checksum_bins hard-codes (kBinGeometry,
  // chosen by the round-1 binning A/B); the last bin: a long segment
  return bin < kBins - 1 ? kBinGeometry[bin] : pick_geometry(uint64_t(1) << 16);
}

SegSpec bin_spec(const SegSpec& whole, const void* list, const uint32_t* meta, int bin) {
  SegSpec sp = whole;
  sp.list = static_cast<const u32x4*>(list) + uint64_t(bin) * whole.n;
  sp.meta = meta;
  sp.bin = bin;
  return sp;
}

}  // namespace icsum
