// icsum_batchv.h — several batches in one launch (k_checksum_batchv,
// k_ipv4_batchv) and their launchers.
#pragma once

#include "icsum_checksum.h"
#include "icsum_ipv4.h"

namespace icsum {
namespace {

// ------------------------------------------------- multi-batch launches ---
// The table of a multi-batch launch, by value in the kernel arguments (the
// block offsets are scanned with scalar loads; a batch's fields are loaded
// from the kernel-argument segment at its index — no scratch copy).
template <typename D>
struct BvTable {
  D b[kMaxBatchv];
  uint32_t block0[kMaxBatchv];  // first block of batch j (ascending; block0[0] = 0)
  uint32_t nblk[kMaxBatchv];
  uint32_t k;
};

// the batch that owns (logical) block blk: block0 is ascending and padded
// with 0xFFFFFFFF past the last batch, so the batch index is the number of
// entries 1..15 at or below blk — one scalar compare per entry, a bitmask and
// s_bcnt1 (the uniform index keeps the descriptor load a scalar load)
template <typename D>
__device__ __forceinline__ uint32_t bv_find(const BvTable<D>& t, uint32_t blk) {
  uint32_t mask = 0;
#pragma unroll
  for (uint32_t q = 1; q < uint32_t(kMaxBatchv); ++q) mask |= blk >= t.block0[q] ? (1u << q) : 0u;
  return __builtin_amdgcn_readfirstlane(uint32_t(__builtin_popcount(mask)));
}

template <int CLS>
__global__ __launch_bounds__(kBlock) void k_checksum_batchv(BvTable<BvSeg> t, const u32x4* __restrict__ zero16,
                                                            uint32_t remap) {
  const uint32_t blk = block_order(remap);  // XCD runs over the whole grid, batches in turn
  const uint32_t j = bv_find(t, blk);
  const BvSeg& b = t.b[j];
  const uint32_t lb = blk - t.block0[j], nb = t.nblk[j];
  const uint32_t* ip = b.init ? b.init : reinterpret_cast<const uint32_t*>(zero16);
  const uint32_t is = b.init ? 1u : 0u;
  const uint8_t* op = reinterpret_cast<const uint8_t*>(zero16);
  SegSrc src{b.offsets, b.stride, b.seg_len, nullptr, nullptr, -1};
  const uint8_t* const bytes = rebase(b.bytes, src);  // the dense class is chosen for aligned bases only
  if constexpr (CLS == kBvDense64)
    checksum_dense_body<4, 4, true, 0>(reinterpret_cast<const u32x4*>(b.bytes), ip, is, b.out, b.n, lb);
  else if constexpr (CLS == kBvTiny)
    checksum_tiny_body<0>(bytes, src, ip, is, op, 0u, zero16, b.out, b.n, lb, nb);
  else if constexpr (CLS == kBvSmall)
    checksum_small_body<4, 2, 2, 0>(bytes, src, ip, is, op, 0u, zero16, b.out, b.n, lb, nb);
  else if constexpr (CLS == kBvLine16)
    checksum_body<16, 8, true, 3, 0>(bytes, src, ip, is, op, 0u, b.out, b.n, lb, nb);
  else
    checksum_body<64, 8, true, 3, 0>(bytes, src, ip, is, op, 0u, b.out, b.n, lb, nb);
}

template <int CLS>
__global__ __launch_bounds__(kBlock) void k_ipv4_batchv(BvTable<BvDgram> t, int mode,
                                                        const uint8_t* __restrict__ zpad, uint32_t remap) {
  const uint32_t blk = block_order(remap);
  const uint32_t j = bv_find(t, blk);
  const BvDgram& b = t.b[j];
  const uint32_t lb = blk - t.block0[j], nb = t.nblk[j];
  if constexpr (CLS == kBvLane1)
    ipv4_body<1, 4, false, 0>(b.dgrams, b.offsets, b.stride, b.dlen, b.n, mode, b.ip_ck, b.tcp_ck, b.status, zpad,
                              lb, nb);
  else if constexpr (CLS == kBvLine16)
    ipv4_body<16, 8, true, 3>(b.dgrams, b.offsets, b.stride, b.dlen, b.n, mode, b.ip_ck, b.tcp_ck, b.status, zpad,
                              lb, nb);
  else
    ipv4_body<64, 8, true, 3>(b.dgrams, b.offsets, b.stride, b.dlen, b.n, mode, b.ip_ck, b.tcp_ck, b.status, zpad,
                              lb, nb);
}

}  // namespace

uint64_t batchv_blocks(int cls, uint64_t n) {
  // segments per block: dense 64 groups x 4 in flight, tiny 256 lanes,
  // small 64 groups x 2 in flight, line grids kBlock / lanes per segment
  const uint64_t per = cls == kBvDense64 || cls == kBvTiny || cls == kBvLane1 ? 256 : cls == kBvSmall ? 128
                       : cls == kBvLine16 ? 16 : 4;
  return (n + per - 1) / per;
}

namespace {
template <typename D>
bool bv_table(const D* b, int k, int cls, BvTable<D>& t, uint64_t& blocks) {
  if (k < 1 || k > kMaxBatchv) return false;
  t = {};
  t.k = uint32_t(k);
  blocks = 0;
  for (int j = k; j < kMaxBatchv; ++j) t.block0[j] = 0xFFFFFFFFu;  // no batch: never at or below a block
  for (int j = 0; j < k; ++j) {
    t.b[j] = b[j];
    const uint64_t nb = batchv_blocks(cls, b[j].n);
    if (nb == 0) return false;
    t.block0[j] = uint32_t(blocks);
    t.nblk[j] = uint32_t(nb);
    blocks += nb;
  }
  return blocks < (uint64_t(1) << 24);
}
}  // namespace

hipError_t launch_checksum_batchv(const BvSeg* b, int k, int cls, const void* zero16, hipStream_t st) {
  BvTable<BvSeg> t;
  uint64_t blocks = 0;
  if (!bv_table(b, k, cls, t, blocks)) return hipErrorInvalidValue;
  const u32x4* z = static_cast<const u32x4*>(zero16);
  const dim3 grid{uint32_t(blocks), 1, 1};
  switch (cls) {
    case kBvDense64: hipLaunchKernelGGL(k_checksum_batchv<kBvDense64>, grid, dim3(kBlock), 0, st, t, z, g_xcd_remap); break;
    case kBvTiny: hipLaunchKernelGGL(k_checksum_batchv<kBvTiny>, grid, dim3(kBlock), 0, st, t, z, g_xcd_remap); break;
    case kBvSmall: hipLaunchKernelGGL(k_checksum_batchv<kBvSmall>, grid, dim3(kBlock), 0, st, t, z, g_xcd_remap); break;
    case kBvLine16: hipLaunchKernelGGL(k_checksum_batchv<kBvLine16>, grid, dim3(kBlock), 0, st, t, z, g_xcd_remap); break;
    case kBvLine64: hipLaunchKernelGGL(k_checksum_batchv<kBvLine64>, grid, dim3(kBlock), 0, st, t, z, g_xcd_remap); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_ipv4_batchv(const BvDgram* b, int k, int cls, int mode, const void* zero16, hipStream_t st) {
  BvTable<BvDgram> t;
  uint64_t blocks = 0;
  if (!bv_table(b, k, cls, t, blocks)) return hipErrorInvalidValue;
  const uint8_t* z = static_cast<const uint8_t*>(zero16);
  const dim3 grid{uint32_t(blocks), 1, 1};
  switch (cls) {
    case kBvLane1: hipLaunchKernelGGL(k_ipv4_batchv<kBvLane1>, grid, dim3(kBlock), 0, st, t, mode, z, g_xcd_remap); break;
    case kBvLine16: hipLaunchKernelGGL(k_ipv4_batchv<kBvLine16>, grid, dim3(kBlock), 0, st, t, mode, z, g_xcd_remap); break;
    case kBvLine64: hipLaunchKernelGGL(k_ipv4_batchv<kBvLine64>, grid, dim3(kBlock), 0, st, t, mode, z, g_xcd_remap); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace icsum
