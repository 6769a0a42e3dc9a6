// icsum_span.h — tile launches of offsets batches (k_span) and the three
// launch_tile_* launchers.
#pragma once

#include "icsum_ipv4.h"
#include "icsum_wrap.h"

namespace icsum {
namespace {

// ------------------------------------------ tile launches (offsets) -------
// An offsets batch is one packed byte stream: segment i = [off[i], off[i+1]).
// The tile launch streams it by position, whatever the segment lengths: no
// lane idles on an ACK-sized segment and no lane group waits on an MTU-sized
// one (the per-segment launches above map one segment to a lane group).
// Segment i's sums over [lo_i, hi_i) are F(hi_i) - F(lo_i), F(x) the sums of
// the stream's bytes below x: exact in uint32 (addition mod 2^32), roles by
// address parity.
//   checksum  lo = start                        (checksum.h:20-41)
//   IPv4/TCP  lo = start + 4 hlen (TCP part)    (ipv4_header.cpp:50, tcp_segment.cpp:11-18)
//   wrap      lo = start + 40 (the payload)     (tcp_over_ip.cpp:69-88)
//   wrap, headers apart: lo = start (segments are payloads), the headers go
//             to an array of their own, 40 contiguous bytes per segment
// k_span below runs it; round 4's k_tile (a block per T segments, each wave
// streaming a quarter of the tile, the points sorted in LDS) is gone since
// round 5 (git c581ecc; profiles/r5k_ab_span_ops.jsonl).
constexpr uint32_t kWinChunks = 256;          // one wave window: 4 KiB, four loads per lane
constexpr int kTileSum = 0, kTileIpv4 = 1, kTileWrap = 2, kTileWrapApart = 3;

// LDS slot of chunk r of a window (16-byte slots): r ^ ((r >> 4) & 3).  The
// window is written as loaded (lane l: chunks 64 u + l, eight contiguous
// lanes per ds_write_b128 group: still conflict-free) and read back four
// consecutive chunks per lane (lane L: 4 L .. 4 L + 3); without the swizzle
// every ds_read_b128 lane group (16 lanes, banks (a / 4) mod 64) of that
// read hits only 4 distinct 16-byte bank groups — 4-way conflicts
// (SQ_LDS_BANK_CONFLICT 15 M cycles per 1 M x 770 B launch,
// profiles/r5_pmc_stream.jsonl); with it each group's 16 lanes cover all 16.
__device__ __forceinline__ uint32_t win_slot(uint32_t r) { return r ^ ((r >> 4) & 3u); }

// inclusive prefix sum over the 64 lanes of a wave: row shifts 1, 2, 4, 8,
// then row 0's total into row 1 and row 2's into row 3, then rows 0-1's into
// rows 2-3
__device__ __forceinline__ uint32_t wave_prefix_incl(uint32_t x) {
  x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xF, 0xF, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xA, 0xF, false);  // row_bcast:15
  x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xC, 0xF, false);  // row_bcast:31
  return x;
}

struct TileArgs {
  // checksum: per-segment initial sums and parities (zero16 + step 0 when absent), u16 or u32 out
  const uint32_t* init;
  const uint8_t* odd;
  uint32_t init_step, odd_step;
  void* out;
  // IPv4 / TCP: mode and the three outputs (each nullable)
  int mode;
  uint16_t* ip_ck;
  uint16_t* tcp_ck;
  uint8_t* status;
  // wrap: the message records; headers apart: the 40-byte headers' array
  const TcpMsg* msgs;
  uint32_t* hdr_out;
};

// ---------------------------------------- wave spans (round 5) -------------
// k_span: every wave on its own.  Wave w owns segments [S w, S w + S) of an
// offsets batch (S <= 63: the dispatch sizes spans from the batch's mean
// length) and streams their bytes [off[i0] & ~15, off[i0 + m]) as
// one range in 4 KiB windows: three register sets, each reloaded as soon as
// its window is in LDS (three windows in flight while one is summed), the
// window written to swizzled LDS slots as loaded and read back four chunks
// per lane, one wave scan per role.  Lane p holds point A = off[i0 + p]
// (p <= m <= S) in registers for the whole span: the window holding it sets
// the lane's F (prefix + masked chunk) — no point lists, loops or LDS buffers
// — and segment t's sums up to its end are F(t + 1), lane t + 1's value one
// shuffle away.  The lo = start operations (checksum; headers-apart wrap)
// take segment t's sums as F(t + 1) - F(t); the others give lane t a second
// point B = lo_t (IPv4: start + 4 IHL, the header's first dword fetched
// before the stream; in-place wrap: start + 40) and take F(t + 1) - F(B).
// No block barrier and no block-level state: a block is four independent
// waves, and the hardware dispatcher balances them over the chip the way it
// does one-shot waves (a persistent or one-tile-per-block grid leaves the
// chip's last waves unbalanced: static tiles 72 %, one-shot waves 82 % of
// 8 TB/s streaming the same 141 MB, profiles/r5_probe_grab.jsonl).
// Every F of a span comes from the wave's single copy of each window, so
// bytes of a neighbouring span's segments that share a boundary chunk (and
// that span's in-place stores into them) cancel out of every difference.
// Per-segment words the outputs need are fetched after the stream (the
// checksum's two ride along it): fewer registers across the window loop.
constexpr uint32_t kSpanSegs = 63;  // most segments per wave: 64 points, one per lane

__device__ __forceinline__ uint64_t shfl_down64(uint64_t v) {
  return uint64_t(uint32_t(__shfl_down(uint32_t(v), 1))) | (uint64_t(uint32_t(__shfl_down(uint32_t(v >> 32), 1))) << 32);
}

// The outputs of a span of m segments [i0, i0 + m) once every lane holds
// F of its point A (fe, fo: the sums of the span's bytes below x) and of its
// point B (ge, go: below lo): segment t = lane t's sums are F(A_{t+1}) -
// F(B_t).  Checksum: init0 / odd0 are the segment's init and parity words.
// Wraps: `stage` is 10 * 64 dwords of the wave's LDS (free once the stream is
// summed).  Every lane of the wave calls it.
template <int OP, int OUT>
__device__ __forceinline__ void span_outputs(uint8_t* __restrict__ bytes, const TileArgs& a, uint32_t lane,
                                             bool valid, uint64_t i, uint64_t i0, uint32_t m, uint64_t x,
                                             uint64_t e, uint64_t lo, bool hdr, uint32_t fe, uint32_t fo,
                                             uint32_t ge, uint32_t go, uint32_t init0, uint32_t odd0,
                                             uint32_t* __restrict__ stage) {
  // segment t's sums up to its end: lane t + 1's F (every lane shuffles,
  // outside the branches below: a shuffle from a lane a branch disables
  // reads nothing defined)
  const uint32_t he = __shfl_down(fe, 1), ho = __shfl_down(fo, 1);
  const uint32_t se = he - ge, so = ho - go;  // sums of [lo, e), roles by address
  if constexpr (OP == kTileSum) {
    if (valid) {
      const uint32_t sum = init0 + combine_roles(se, so, (uint32_t(x) ^ odd0) & 1u);
      if (OUT == 0)
        static_cast<uint16_t*>(a.out)[i] = fold_value(sum);
      else
        static_cast<uint32_t*>(a.out)[i] = sum;
    }
  } else if constexpr (OP == kTileIpv4) {
    // the header and the TCP fields at the real start of the TCP part (after
    // the stream: no window load waits behind them)
    if (valid) {
      const uint32_t* last = last_dword(bytes + e);
      Hdr h{};
      uint32_t tf0 = 0, tf1 = 0;
      if (hdr) {
        h = load_hdr(bytes + x, last);
        if (e - lo >= 18) load_tcp_fields(bytes + lo, last, tf0, tf1);
      }
      ipv4_result(bytes, x, e, lo, hdr, h, tf0, tf1, combine_roles(se, so, uint32_t(lo) & 1u), a.mode, i, a.ip_ck,
                  a.tcp_ck, a.status);
    }
  } else {
    // the message record, then the header into the wave's (now idle) window
    // slots: 10 dwords per segment, the span's m headers contiguous
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.msgs + i);
    uint32_t w[7];
#pragma unroll
    for (uint32_t k = 0; k < 7; ++k) w[k] = rec[k];
    const bool ok = valid && (OP == kTileWrapApart || e - x >= 40);
    if (valid) {
      uint32_t ipc = 0, tcv = 0;
      wrap_header(u32x4{w[0], w[1], w[2], w[3]}, w[4], w[5], w[6] & 0xffffu, e - lo,
                  combine_roles(se, so, uint32_t(lo) & 1u), stage + lane * 10u, ipc, tcv);
      if (a.ip_ck) a.ip_ck[i] = ok ? uint16_t(ipc) : uint16_t(0);
      if (a.tcp_ck) a.tcp_ck[i] = ok ? uint16_t(tcv) : uint16_t(0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if constexpr (OP == kTileWrapApart) {
      // the span's 10 m header dwords are one contiguous run of hdr_out:
      // coalesced 256-byte stores instead of 40-byte strides per lane
      uint32_t* const dst = a.hdr_out + i0 * 10;
#pragma unroll
      for (uint32_t j = 0; j < 10; ++j) {
        const uint32_t q = j * 64u + lane;
        if (q < m * 10u) dst[q] = stage[q];
      }
    } else {
      // in place: dword q of the span = dword q % 10 of segment q / 10
      // (neighbouring lanes, neighbouring bytes); its start and whether it
      // holds a header come from lane q / 10 (every lane shuffles)
      const uint32_t okw = ok ? 1u : 0u;
#pragma unroll 2
      for (uint32_t j = 0; j < 10; ++j) {
        const uint32_t q = j * 64u + lane, d = q / 10u, k = q - d * 10u;
        const uint32_t src = d < 64u ? d : 63u;
        const uint64_t ds = uint64_t(uint32_t(__shfl(uint32_t(x), int(src)))) |
                            (uint64_t(uint32_t(__shfl(uint32_t(x >> 32), int(src)))) << 32);
        const uint32_t dok = uint32_t(__shfl(okw, int(src)));
        if (d < m && dok) {
          const uint32_t v = stage[q];
          uint8_t* q8 = bytes + ds + 4u * k;
          if ((reinterpret_cast<uintptr_t>(q8) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(q8) = v;
          } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) q8[b] = uint8_t(v >> (8 * b));
          }
        }
      }
    }
  }
}

template <int OP, int OUT, bool STRIDE>
__global__ __launch_bounds__(kBlock) void k_span(uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off,
                                                 uint64_t n, uint32_t S, TileArgs a, uint32_t remap,
                                                 const u32x4* __restrict__ zero16) {
  constexpr bool TWO = OP == kTileIpv4 || OP == kTileWrap;  // a second point per lane: lo_t
  constexpr uint32_t kWaves = kBlock / 64;
  __shared__ uint32_t s_pre[kWaves][kWinChunks][2];
  __shared__ u32x4 s_raw[kWaves][kWinChunks];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t nspans = (n + S - 1) / S;
  const uint32_t bsh = frame_shift(bytes);  // the kernel's frame (icsum_device.h): points and windows absolute
  bytes -= bsh;
  // one span per wave; STRIDE (batches of more spans than 2^24 blocks hold):
  // grid-stride beyond the grid.  Wave-uniform, no block barrier anywhere.
  auto span_body = [&](uint64_t span) {
  const uint64_t i0 = span * S;
  const uint32_t m = uint32_t(n - i0 < S ? n - i0 : S);
  const bool valid = lane < m;
  const uint64_t i = i0 + (valid ? lane : 0u);  // lanes >= m: a harmless copy of segment 0
  // point A (one load per lane) and, for the checksum, the per-segment words —
  // in flight before the first window is requested
  const uint64_t x = off[i0 + (lane <= m ? lane : m)] + bsh;
  uint32_t w[2] = {0u, 0u};  // checksum: the segment's init and parity
  if constexpr (OP == kTileSum) {
    w[0] = a.init[i * a.init_step];
    w[1] = a.odd[i * a.odd_step];
  }
  // the span's byte range: two scalar loads at wave-uniform indices (the
  // stream's addresses wait for the scalar cache, not for the vector load)
  const uint64_t first = off[i0] + bsh, tend = off[i0 + m] + bsh;
  // segment t = [x, e): e is lane t + 1's point (taken by every lane).  IPv4
  // takes it before the stream, for the header's first dword (the IHL); the
  // other operations after the stream is requested
  uint64_t e = 0;
  bool hdr = false;
  uint32_t d0 = 0, d0sh = 0;  // the dword holding header byte 0 and that byte's place in it
  if constexpr (OP == kTileIpv4) {
    e = shfl_down64(x);
    hdr = valid && e - x >= 20;
    const uint8_t* hp = hdr ? bytes + x : reinterpret_cast<const uint8_t*>(zero16);
    d0sh = uint32_t(reinterpret_cast<uintptr_t>(hp) & 3u);
    d0 = *reinterpret_cast<const uint32_t*>(hp - d0sh);
  }
  // the windows start on the 128-byte line (of `bytes`) holding the first
  // byte, so each 1 KiB load instruction covers 8 whole lines, not 9 partial
  // ones; the chunks below `first` enter every F of the span alike and cancel
  const uint64_t a0c = (first >> 7) << 3;
  const uint64_t nch = tend > (a0c << 4) ? ((tend + 15) >> 4) - a0c : 0;
  const uint64_t nw = (nch + kWinChunks - 1) / kWinChunks;
  // three register sets per wave, each reloaded as soon as its window is in
  // LDS: up to three windows in flight (two sets at 6 waves / SIMD, and three
  // forced to 5 waves / SIMD by spilling, measured equal or slower:
  // profiles/r5y_ab_span_sets_waves.jsonl)
  constexpr uint32_t kSets = 3;
  const uint64_t nwin3 = nw ? (nw + kSets - 1) / kSets * kSets : kSets;  // whole rounds of the sets
  const uint32_t voff = lane * 16u;
  auto load_win = [&](uint64_t k, u32x4 (&v)[4]) {
    const uint64_t c0 = k * kWinChunks;
    const uint64_t left = nch > c0 ? nch - c0 : 0;
    const uint32_t len = uint32_t(left < kWinChunks ? left : kWinChunks);
    const u32x4* pw = reinterpret_cast<const u32x4*>(bytes) + a0c + (len ? c0 : 0);
#ifdef ICSUM_BOUNDS_CHECK
    if (len) {
      const uint8_t* lo8 = bytes + (a0c << 4);
      ICS_CHECK16(pw, lo8, lo8 + (nch << 4));
      ICS_CHECK16(pw + len - 1, lo8, lo8 + (nch << 4));
    }
#endif
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(pw), 0, int(len * 16u), 0x00020000);
#pragma unroll
    for (int u = 0; u < 4; ++u)  // aux 2: non-temporal
      v[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, u * 1024, 2));
  };
  u32x4 b0[4], b1[4], b2[4];
  // in this order: the loop consumes b0 first, and vmcnt retires loads in issue order
  load_win(0, b0);
  __builtin_amdgcn_sched_barrier(0);
  load_win(1, b1);
  __builtin_amdgcn_sched_barrier(0);
  load_win(2, b2);
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (OP != kTileIpv4) e = shfl_down64(x);
#ifdef ICSUM_BOUNDS_CHECK
  if (valid && e < x) bounds_fail(kBoundsOffsets, i);
#endif
  // point B, once the windows are out: IPv4 past the header (options skipped,
  // ipv4_header.cpp:50), the in-place wrap past the 40 header bytes it rewrites
  auto point_b = [&](uint64_t e_) {
    uint64_t lo_ = x;
    if constexpr (OP == kTileIpv4) {
      uint64_t o = 4u * ((d0 >> (8u * d0sh)) & 0x0fu);  // the byte in the frame of the load
      if (o < 20) o = 20;
      if (hdr && o > e_ - x) o = e_ - x;
      lo_ = hdr ? x + o : e_;
    } else if constexpr (OP == kTileWrap) {
      lo_ = valid && e_ - x >= 40 ? x + 40 : e_;
    }
    return lo_;
  };
  const uint64_t lo = point_b(e);
  // the lane's points: chunk (span-relative, 32 bits) and byte; lanes past m
  // hold no A, lanes >= m no B
  const uint32_t pc = lane <= m ? uint32_t((x >> 4) - a0c) : ~0u;
  const uint32_t pb = uint32_t(x) & 15u;
  const uint32_t qc = TWO && valid ? uint32_t((lo >> 4) - a0c) : ~0u;
  const uint32_t qb = uint32_t(lo) & 15u;
  uint32_t ce = 0, co = 0;  // the span's sums so far
  uint32_t fe = 0, fo = 0;  // F of point A (set by the window holding it)
  uint32_t ge = 0, go = 0;  // F of point B
  // F at a point inside window [c0, c1): its chunk's prefix + the chunk's bytes below it
  auto point_F = [&](uint32_t c, uint32_t b, uint64_t c0, uint32_t& fe_, uint32_t& fo_) {
    const uint32_t k2 = uint32_t(c - c0);
    fe_ = s_pre[wv][k2][0];
    fo_ = s_pre[wv][k2][1];
    acc_chunk(s_raw[wv][win_slot(k2)] & byte_range_mask(0u, b), fe_, fo_);
  };
  auto window = [&](uint64_t k, u32x4 (&v)[4]) {
    const uint64_t c0 = k * kWinChunks;
    const bool live = c0 < nch;  // uniform; else a padding window
    if (live) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s_raw[wv][win_slot(uint32_t(u) * 64u + lane)] = v[u];
    }
    load_win(k + kSets, v);  // the registers are free: window k + kSets goes out now (one load site)
    if (!live) return;
#ifdef ICSUM_SPAN_PROBE_STREAM_ONLY
    // diagnostic build only (tools/probe/span_probe.hip): the loads, the LDS
    // writes and one read back per lane, no scan, prefix or points (results
    // wrong, time only)
    {
      const u32x4 r = s_raw[wv][win_slot(4u * lane)];
      ce += r.x ^ r.y ^ r.z ^ r.w;
      __builtin_amdgcn_wave_barrier();
      return;
    }
#endif
    const uint64_t c1 = nch - c0 < kWinChunks ? nch : c0 + kWinChunks;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint32_t pe[4], po[4], te = 0, to = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t ev = 0, od = 0;
      acc_chunk(s_raw[wv][win_slot(4u * lane + uint32_t(j))], ev, od);
      pe[j] = te;
      po[j] = to;
      te += ev;
      to += od;
    }
    const uint32_t ie = wave_prefix_incl(te), io = wave_prefix_incl(to);
    const uint32_t xe = ce + ie - te, xo = co + io - to;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s_pre[wv][4u * lane + uint32_t(j)][0] = xe + pe[j];
      s_pre[wv][4u * lane + uint32_t(j)][1] = xo + po[j];
    }
    ce += __builtin_amdgcn_readlane(ie, 63);
    co += __builtin_amdgcn_readlane(io, 63);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (pc >= c0 && pc < c1) point_F(pc, pb, c0, fe, fo);  // (~0u: no point, past any window)
    if constexpr (TWO) {
      if (qc >= c0 && qc < c1) point_F(qc, qb, c0, ge, go);
    }
    __builtin_amdgcn_wave_barrier();  // the next window rewrites s_pre / s_raw
  };
  // wave-uniform; nwin3 >= kSets, so a do-while: no zero-trip test for the
  // compiler to sink the first three windows' loads behind
  uint64_t k = 0;
  do {
    window(k, b0);
    window(k + 1, b1);
    window(k + 2, b2);
    k += kSets;
  } while (k < nwin3);
  // a point at the aligned end of the last chunk: every byte is below it
  if (lane <= m && pc >= nch) {
    fe = ce;
    fo = co;
  }
  if constexpr (TWO) {
    if (valid && qc >= nch) {
      ge = ce;
      go = co;
    }
  } else {
    ge = fe;
    go = fo;
  }
  span_outputs<OP, OUT>(bytes, a, lane, valid, i, i0, m, x, e, lo, hdr, fe, fo, ge, go, w[0], w[1],
                        reinterpret_cast<uint32_t*>(&s_raw[wv][0]));
  __builtin_amdgcn_wave_barrier();  // the next span rewrites s_pre / s_raw
  };
  const uint64_t span0 = uint64_t(block_order(remap)) * kWaves + wv;
  if constexpr (STRIDE) {
    for (uint64_t span = span0; span < nspans; span += uint64_t(gridDim.x) * kWaves) span_body(span);
  } else if (span0 < nspans) {
    span_body(span0);
  }
}

// k_span: one wave per S segments, four independent waves per block
template <int OP, int OUT>
hipError_t launch_span_t(const SegSpec& sp, const TileArgs& a, uint32_t S, hipStream_t st, uint32_t max_blocks) {
  if (!sp.offsets || sp.list || sp.n == 0 || S == 0 || S > kSpanSegs) return hipErrorInvalidValue;
  const uint64_t waves = (sp.n + S - 1) / S;
  const uint64_t blocks = (waves + kBlock / 64 - 1) / (kBlock / 64);
  const uint64_t cap = max_blocks && max_blocks < kMaxGridBlocks ? max_blocks : kMaxGridBlocks;
  uint8_t* const bytes = const_cast<uint8_t*>(sp.bytes);
  const u32x4* const z = static_cast<const u32x4*>(sp.zero16);
  if (blocks > cap)  // more spans than one grid: grid-stride
    hipLaunchKernelGGL((k_span<OP, OUT, true>), dim3(uint32_t(cap)), dim3(kBlock), 0, st, bytes,
                       sp.offsets, sp.n, S, a, g_xcd_remap, z);
  else
    hipLaunchKernelGGL((k_span<OP, OUT, false>), dim3(uint32_t(blocks)), dim3(kBlock), 0, st, bytes, sp.offsets,
                       sp.n, S, a, g_xcd_remap, z);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_tile_checksum(const SegSpec& sp, const uint32_t* init, const uint8_t* odd, void* out, int out_kind,
                                uint32_t S, hipStream_t st, uint32_t max_blocks) {
  TileArgs a{};
  const SegWords w = seg_words(init, odd, sp.zero16);
  a.init = w.ip;
  a.odd = w.op;
  a.init_step = w.is;
  a.odd_step = w.os;
  a.out = out;
  return with_out(out_kind, [&](auto OUT) { return launch_span_t<kTileSum, OUT()>(sp, a, S, st, max_blocks); });
}

hipError_t launch_tile_ipv4(const SegSpec& sp, int mode, uint16_t* ip_ck, uint16_t* tcp_ck, uint8_t* status,
                            uint32_t S, hipStream_t st, uint32_t max_blocks) {
  TileArgs a{};
  a.mode = mode;
  a.ip_ck = ip_ck;
  a.tcp_ck = tcp_ck;
  a.status = status;
  return launch_span_t<kTileIpv4, 0>(sp, a, S, st, max_blocks);
}

hipError_t launch_tile_wrap(const SegSpec& sp, const TcpMsg* msgs, uint32_t* hdr_out, uint16_t* ip_ck,
                            uint16_t* tcp_ck, uint32_t S, hipStream_t st, uint32_t max_blocks) {
  TileArgs a{};
  a.msgs = msgs;
  a.hdr_out = hdr_out;
  a.ip_ck = ip_ck;
  a.tcp_ck = tcp_ck;
  return hdr_out ? launch_span_t<kTileWrapApart, 0>(sp, a, S, st, max_blocks)
                 : launch_span_t<kTileWrap, 0>(sp, a, S, st, max_blocks);
}

}  // namespace icsum
