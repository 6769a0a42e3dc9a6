// icsum_scatter.h — k_copy_pieces and its launcher: the data plane of the
// receive streams (include/icsum.h, ics_copy_pieces / ics_rx_stream_receive_batch).
// m pieces {src, dst, len} (ics_copy_piece, 16 bytes) in device memory; piece p
// copies src_base[src .. src + len) to dst_base[dst .. dst + len), an unaligned
// gather / scatter with a byte count, a source residue and a destination
// residue per piece.  The host planner is csrc/icsum_rxstream.cpp.
#pragma once

#include "icsum_common.h"

namespace icsum {
namespace {

// Work split: a group of 16 lanes owns one piece and walks the piece's
// DESTINATION blocks (aligned 16 bytes), lane l taking blocks l, l + 16, ...:
// a wave has four pieces in flight, a block sixteen.  An MTU payload (1460 B,
// 92 blocks) is six steps of a group, a 100-byte piece one step of seven
// lanes; the longest piece (65 495 B) is 256 steps of one group while the
// other groups of its wave move on to their next pieces' blocks only at the
// next grid-stride trip — the price of one shape for every length (k_span's
// packed windows would level that; DESIGN.md §14 says why it was not taken).
//
// Per destination block at ring offset B (in the frame of the 16-byte-aligned
// address at or below dst_base): its bytes [lo, hi) belong to the piece, and
// byte j comes from source address S + j, S = B + (src - dst).  S & 15 is the
// residue difference r, the same for every block of the piece: the 16 bytes
// are funnel-shifted (alignbyte, as row_take does) out of the two aligned
// source blocks at S & ~15 and + 16.  Either block address is clamped into the
// piece's envelope [src & ~15, (src + len + 15) & ~15): a needed byte always
// lies in an unclamped block, a clamped block only feeds bytes outside
// [lo, hi) — nothing is read outside the blocks that hold the piece, and the
// last block's load is clamped, not skipped.
// Stores: a block wholly inside the piece is one aligned dwordx4 store; a
// partial head or tail block (which a neighbouring piece, written by another
// group, may share) is stored dword by dword where the dword is wholly the
// piece's and byte by byte elsewhere — never read, merged and written back.  A
// piece shorter than 16 bytes is one partial block (or two) on the same path.
// Indexing: source addressing 64-bit (S is signed: the head block's S may lie
// below the source base's frame), ring offsets 32-bit (dst_bytes <= 2^31), the
// grid stride over pieces 64-bit.
struct alignas(8) CopyPiece {  // ics_copy_piece
  uint64_t src;
  uint32_t dst, len;
};
static_assert(sizeof(CopyPiece) == 16, "ics_copy_piece layout");
constexpr uint32_t kPieceLanes = 16;
constexpr uint32_t kPiecesPerBlock = kBlock / kPieceLanes;

__global__ __launch_bounds__(kBlock) void k_copy_pieces(const uint8_t* __restrict__ src_base,
                                                        [[maybe_unused]] uint64_t src_bytes,
                                                        uint8_t* __restrict__ dst_base,
                                                        [[maybe_unused]] uint32_t dst_bytes,
                                                        const CopyPiece* __restrict__ pieces, uint64_t m) {
  const uint32_t ssh = frame_shift(src_base), dsh = frame_shift(dst_base);
  src_base -= ssh;
  dst_base -= dsh;
  const uint32_t sub = threadIdx.x & (kPieceLanes - 1u);
  const uint64_t step = uint64_t(gridDim.x) * kPiecesPerBlock;
  for (uint64_t p = uint64_t(blockIdx.x) * kPiecesPerBlock + (threadIdx.x / kPieceLanes); p < m; p += step) {
    const CopyPiece pc = pieces[p];  // 16 bytes, the same address in all 16 lanes
    const uint32_t len = pc.len;
    if (len == 0u) continue;
    const uint64_t s = pc.src + ssh;
    const uint32_t d = pc.dst + dsh;
    const uint32_t a0 = d & ~15u;
    const uint32_t nblk = (d + len + 15u - a0) >> 4;
    const int64_t e0 = int64_t(s & ~uint64_t(15));                         // the envelope's first block
    const int64_t e1 = int64_t((s + len + 15u) & ~uint64_t(15)) - 16;      // ... and its last
    const int64_t rel = int64_t(s) - int64_t(d);
    const uint32_t r = uint32_t(rel) & 15u, q = r >> 2, sh = r & 3u;
#ifdef ICSUM_BOUNDS_CHECK
    // the envelope inside the source buffer's blocks, the piece inside the ring
    if (s + len > uint64_t(ssh) + src_bytes || s + len < s) {
      bounds_fail(kBoundsPieceLoad, reinterpret_cast<unsigned long long>(src_base + s + len));
      continue;
    }
    if (uint64_t(d) + len > uint64_t(dsh) + dst_bytes) {
      bounds_fail(kBoundsPieceStore, uint64_t(pc.dst) + len);
      continue;
    }
#endif
    for (uint32_t k = sub; k < nblk; k += kPieceLanes) {
      const uint32_t B = a0 + (k << 4);
      const int64_t sa = (int64_t(B) + rel) & ~int64_t(15);
      const int64_t la = sa < e0 ? e0 : (sa > e1 ? e1 : sa);
      const int64_t sb = sa + 16;
      const int64_t lb = sb < e0 ? e0 : (sb > e1 ? e1 : sb);
#ifdef ICSUM_BOUNDS_CHECK
      {
        const int64_t top = int64_t((uint64_t(ssh) + src_bytes + 15u) & ~uint64_t(15));
        if (la < 0 || la + 16 > top) bounds_fail(kBoundsPieceLoad, reinterpret_cast<unsigned long long>(src_base + la));
        if (lb < 0 || lb + 16 > top) bounds_fail(kBoundsPieceLoad, reinterpret_cast<unsigned long long>(src_base + lb));
      }
#endif
      const u32x4 va = *reinterpret_cast<const u32x4*>(src_base + la);
      const u32x4 vb = *reinterpret_cast<const u32x4*>(src_base + lb);
      // five consecutive dwords from dword q of {va, vb}, then the byte shift
      const uint32_t t0 = q == 0u ? va.x : q == 1u ? va.y : q == 2u ? va.z : va.w;
      const uint32_t t1 = q == 0u ? va.y : q == 1u ? va.z : q == 2u ? va.w : vb.x;
      const uint32_t t2 = q == 0u ? va.z : q == 1u ? va.w : q == 2u ? vb.x : vb.y;
      const uint32_t t3 = q == 0u ? va.w : q == 1u ? vb.x : q == 2u ? vb.y : vb.z;
      const uint32_t t4 = q == 0u ? vb.x : q == 1u ? vb.y : q == 2u ? vb.z : vb.w;
      u32x4 o;
      o.x = __builtin_amdgcn_alignbyte(t1, t0, sh);
      o.y = __builtin_amdgcn_alignbyte(t2, t1, sh);
      o.z = __builtin_amdgcn_alignbyte(t3, t2, sh);
      o.w = __builtin_amdgcn_alignbyte(t4, t3, sh);
      const uint32_t lo = d > B ? d - B : 0u;
      const uint32_t hi = d + len - B < 16u ? d + len - B : 16u;
      uint8_t* const out = dst_base + B;
      if (lo == 0u && hi == 16u) {
        *reinterpret_cast<u32x4*>(out) = o;
      } else {
        const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          if (lo <= 4u * i && hi >= 4u * i + 4u) {
            *reinterpret_cast<uint32_t*>(out + 4u * i) = w[i];
          } else {
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b)
              if (4u * i + b >= lo && 4u * i + b < hi) out[4u * i + b] = uint8_t(w[i] >> (8u * b));
          }
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_copy_pieces(const uint8_t* src, uint64_t src_bytes, uint8_t* dst, uint32_t dst_bytes,
                              const void* pieces, uint64_t m, hipStream_t st) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(k_copy_pieces, dim3(ew_blocks(m * kPieceLanes)), dim3(kBlock), 0, st, src, src_bytes, dst,
                     dst_bytes, static_cast<const CopyPiece*>(pieces), m);
  return hipGetLastError();
}

}  // namespace icsum
