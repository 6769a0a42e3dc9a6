// icsum_unwrap.h — message records from a datagram batch (k_tcp_unwrap) and
// its launcher: what TCPOverIPv4Adapter::unwrap_tcp_in_ip
// (util/tcp_over_ip/tcp_over_ip.cpp:14-64) and TCPSegment::parse
// (util/tcp_segment/tcp_segment.cpp:25-65) read out of a datagram's bytes, one
// 40-byte ics_tcp_rx (include/icsum.h) per datagram.  The checksums are not
// this kernel's: it runs behind the VERIFY launch and reads that launch's
// status bytes.  The host restatement is csrc/icsum_unwrap.cpp.
#pragma once

#include "icsum_hdrpass.h"

namespace icsum {
namespace {

// A header-only pass in rows (rows_load / row_take, icsum_hdrpass.h): a wave
// takes 64 consecutive datagrams per pass.  Speculating hlen 5, the row holds
// the IPv4 header and TCP bytes 0..15; the parsing lane reads its status byte
// and builds the record.  A datagram with IPv4 options (rare) loads its TCP
// dwords at 4 * hlen itself, the fifth clamped to the datagram's last dword,
// as load_tcp_fields does.  `parsed` below holds only when 4 * hlen + 20 <=
// length, whatever the status byte says.
// Store: the wave stages its 64 records in the LDS rows it has just read (ten
// dwords each) and stores them as 640 consecutive dwords.
__global__ __launch_bounds__(kBlock) void k_tcp_unwrap(const uint8_t* __restrict__ dg,
                                                       const uint64_t* __restrict__ offsets, uint64_t stride,
                                                       uint64_t dlen, uint64_t n,
                                                       const uint8_t* __restrict__ status,
                                                       uint32_t* __restrict__ recs,
                                                       const uint32_t* __restrict__ zpad) {
  constexpr uint32_t kRec = 10;
  __shared__ uint32_t raw[kBlock / 64][kRowsPerWave * kRow];
  const uint32_t lane64 = threadIdx.x & 63u;
  uint32_t* const rw = raw[threadIdx.x >> 6];
  const uint64_t step = uint64_t(gridDim.x) * kBlock;
  const uint32_t bsh = frame_shift(dg);
  dg -= bsh;
  for (uint64_t g0 = uint64_t(blockIdx.x) * kBlock; g0 < n; g0 += step) {  // uniform per block
    const uint64_t wbase = g0 + (threadIdx.x >> 6) * kRowsPerWave;
    rows_load<20>(dg, offsets, stride, dlen, n, bsh, wbase, lane64, zpad, rw);
    // ---- parse: lane l has datagram wbase + l
    const uint64_t i = wbase + lane64;
    const bool valid = i < n;
    uint64_t s, e;
    seg_bounds(offsets, stride, dlen, valid ? i : n - 1, s, e, bsh);
    const uint64_t len = item_len(s, e);
    const bool hdr = valid && len >= 20;
    const uint32_t st = valid ? status[i] : 0u;
    uint32_t f[9];  // f[5..8] are TCP bytes 0..15 when hlen is 5
    row_take(rw, lane64, hdr, s, f);
    const uint32_t hlen = f[0] & 0x0fu, hl = 4u * hlen;
    // PARSED (include/icsum.h), and the bytes it promises are there: the header
    // and 20 bytes of TCP behind it
    const bool parsed = hdr && (st & 7u) == 7u && hlen >= 5u && uint64_t(hl) + 20u <= len;
    uint32_t t0 = f[5], t1 = f[6], t2 = f[7], t3 = f[8];
    if (parsed && hlen != 5u) {  // IPv4 options: TCP bytes 0..15 at 4 * hlen, five aligned dwords
      const uint8_t* p = dg + s + hl;
      const uint32_t tsh = uint32_t(reinterpret_cast<uintptr_t>(p) & 3u);
      const uint32_t* q = reinterpret_cast<const uint32_t*>(p - tsh);
      const uint32_t* last = last_dword(dg + e);
#ifdef ICSUM_BOUNDS_CHECK
      if (q + 3 > last) bounds_fail(kBoundsHeader, reinterpret_cast<unsigned long long>(q + 3));
#endif
      const uint32_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3];
      const uint32_t x4 = *(q + 4 < last ? q + 4 : last);
      t0 = __builtin_amdgcn_alignbyte(x1, x0, tsh);
      t1 = __builtin_amdgcn_alignbyte(x2, x1, tsh);
      t2 = __builtin_amdgcn_alignbyte(x3, x2, tsh);
      t3 = __builtin_amdgcn_alignbyte(x4, x3, tsh);
    }
    // t3: TCP bytes 12..15 as they lie — data offset, flags, window (big-endian)
    const uint32_t doff = (t3 & 0xffu) >> 4, flags = (t3 >> 8) & 0x17u;
    const uint64_t po64 = uint64_t(hl) + 4u * doff;
    const uint32_t pay_off = uint32_t(po64 < len ? po64 : len);
    wave_lds_sync();  // every lane has read its row: the rows become the staging area
    uint32_t* rec = rw + lane64 * kRec;
    rec[0] = parsed ? bswap32(f[3]) : 0u;                                        // src
    rec[1] = parsed ? bswap32(f[4]) : 0u;                                        // dst
    rec[2] = parsed ? bswap32(t1) : 0u;                                          // seqno
    rec[3] = parsed && (flags & 0x10u) ? bswap32(t2) : 0u;                       // ackno (tcp_segment.cpp:42-45)
    rec[4] = parsed ? ((t0 & 0x00ff00ffu) << 8) | ((t0 >> 8) & 0x00ff00ffu) : 0u;  // src_port, dst_port
    rec[5] = parsed ? (((t3 >> 16) & 0xffu) << 8) | (t3 >> 24) | (flags << 16) | ((f[2] & 0xffu) << 24) : 0u;
    rec[6] = parsed ? ((f[1] & 0xffu) << 8) | ((f[1] >> 8) & 0xffu) : 0u;        // id, reserved
    rec[7] = parsed ? pay_off : 0u;
    rec[8] = parsed ? uint32_t(len - pay_off) : 0u;
    rec[9] = st;  // status, reserved[3]
    wave_store<kRec>(rw, recs, wbase, n, lane64);
    __builtin_amdgcn_wave_barrier();  // the next pass rewrites the wave's LDS
  }
}

}  // namespace

hipError_t launch_tcp_unwrap(const SegSpec& sp, const uint8_t* status, uint32_t* recs, hipStream_t st) {
  hipLaunchKernelGGL(k_tcp_unwrap, dim3(ew_blocks(sp.n)), dim3(kBlock), 0, st, sp.bytes, sp.offsets, sp.stride,
                     sp.seg_len, sp.n, status, recs, static_cast<const uint32_t*>(sp.zero16));
  return hipGetLastError();
}

}  // namespace icsum
