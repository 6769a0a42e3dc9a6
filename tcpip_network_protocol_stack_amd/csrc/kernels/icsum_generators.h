// icsum_generators.h — the synthetic-workload generators of icsum_workload.h
// and their launchers.
#pragma once

#include "icsum_common.h"

namespace icsum {
namespace {

// ------------------------------------------------- workload spec ---------
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t sm64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t spec_word(uint64_t seed, uint64_t c) {
  return sm64(seed + (c + 1) * kGolden);
}

// Fast path: pos0 % 8 == 0 and d 16-byte aligned -> 16 bytes per thread.
__global__ void k_fill16(u32x4* __restrict__ d, uint64_t nvec, uint64_t seed, uint64_t w0) {
  ICS_GRID_STRIDE(i, nvec) {
  const uint64_t a = spec_word(seed, w0 + 2 * i), b = spec_word(seed, w0 + 2 * i + 1);
  d[i] = u32x4{uint32_t(a), uint32_t(a >> 32), uint32_t(b), uint32_t(b >> 32)};
  }
}

__global__ void k_fill1(uint8_t* __restrict__ d, uint64_t n, uint64_t seed, uint64_t pos0) {
  ICS_GRID_STRIDE(j, n) {
    const uint64_t p = pos0 + j;
    d[j] = uint8_t(spec_word(seed, p >> 3) >> (8 * (p & 7)));
  }
}

__device__ __forceinline__ void spec_addrs(uint64_t seed, uint64_t i, uint32_t& src, uint32_t& dst) {
  const uint64_t m = spec_word(seed ^ 0xA5A5A5A5A5A5A5A5ull, i);
  src = 0x0A000000u | uint32_t(m & 0xFFFFFFu);
  dst = 0x0A000000u | uint32_t((m >> 24) & 0xFFFFFFu);
}

__global__ void k_pseudo_inits(uint32_t* __restrict__ init, const uint64_t* __restrict__ offsets,
                               uint64_t seg_len, uint64_t n, uint64_t seed, uint64_t index0) {
  ICS_GRID_STRIDE(i, n) {
  const uint64_t L = offsets ? offsets[i + 1] - offsets[i] : seg_len;
  uint32_t s, d;
  spec_addrs(seed, index0 + i, s, d);
  init[i] = (s >> 16) + (s & 0xffffu) + (d >> 16) + (d & 0xffffu) + 6u + uint32_t(L & 0xffffu);
  }
}

__global__ void k_ipv4_tcp_headers(uint8_t* __restrict__ dg, uint64_t stride, uint64_t dlen,
                                   uint64_t n, uint64_t seed, uint64_t index0) {
  ICS_GRID_STRIDE(i, n) {
  uint8_t* d = dg + i * stride;
  const uint64_t id = index0 + i;
  uint32_t s, t;
  spec_addrs(seed, id, s, t);
  d[0] = 0x45;
  d[1] = 0;
  d[2] = uint8_t(dlen >> 8);
  d[3] = uint8_t(dlen);
  d[4] = uint8_t(id >> 8);
  d[5] = uint8_t(id);
  d[6] = 0x40;
  d[7] = 0;
  d[8] = 64;
  d[9] = 6;
  for (int k = 0; k < 4; ++k) {
    d[12 + k] = uint8_t(s >> (24 - 8 * k));
    d[16 + k] = uint8_t(t >> (24 - 8 * k));
  }
  if (dlen >= 40) {
    d[32] = 0x50;
    d[33] = 0x10;
    d[38] = 0;
    d[39] = 0;
  }
  }
}

}  // namespace

hipError_t launch_fill_bytes(uint8_t* d, uint64_t nbytes, uint64_t seed, uint64_t pos0,
                             hipStream_t st) {
  if (nbytes == 0) return hipSuccess;
  if ((pos0 & 7) == 0 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
    const uint64_t nvec = nbytes / 16;
    if (nvec) {
      hipLaunchKernelGGL(k_fill16, dim3(ew_blocks(nvec)), dim3(kBlock), 0, st,
                         reinterpret_cast<u32x4*>(d), nvec, seed, pos0 >> 3);
    }
    const uint64_t done = nvec * 16, rest = nbytes - done;
    if (rest)
      hipLaunchKernelGGL(k_fill1, dim3(1), dim3(kBlock), 0, st, d + done, rest, seed, pos0 + done);
  } else {
    hipLaunchKernelGGL(k_fill1, dim3(ew_blocks(nbytes)), dim3(kBlock), 0, st, d, nbytes, seed, pos0);
  }
  return hipGetLastError();
}

hipError_t launch_pseudo_inits(uint32_t* init, const uint64_t* offsets, uint64_t seg_len,
                               uint64_t n, uint64_t seed, uint64_t index0, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pseudo_inits, dim3(ew_blocks(n)), dim3(kBlock), 0, st,
                     init, offsets, seg_len, n, seed, index0);
  return hipGetLastError();
}

hipError_t launch_ipv4_tcp_headers(uint8_t* d, uint64_t stride, uint64_t dgram_len, uint64_t n,
                                   uint64_t seed, uint64_t index0, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_ipv4_tcp_headers, dim3(ew_blocks(n)), dim3(kBlock), 0,
                     st, d, stride, dgram_len, n, seed, index0);
  return hipGetLastError();
}

}  // namespace icsum
