// icsum_tick.h — per-tick host calls: the one-block k_tick and the resident
// k_tick_server, with their launchers.
#pragma once

#include "icsum_ipv4.h"
#include "icsum_wrap.h"

namespace icsum {
namespace {

// ------------------------------------------------- per-tick host calls ----
// A zero-copy host call of at most kTickSegs segments with offsets (a TUN or
// socket loop's tick, INTEGRATION.md §4 "Per-tick host batches"): one block,
// a 16-lane group per segment, the n + 1 offsets in the kernel arguments.  The
// grid-wide kernels read them from the caller's page-locked offsets, a
// dependent PCIe round trip ahead of the first payload load (1.3-1.6 us of a
// 10-13 us call, profiles/r5_tick_latency.jsonl); here the first loads are
// the payload bytes.  OP 0: checksum (u16 value), 1: the fused IPv4/TCP item.
template <int OP>
__global__ __launch_bounds__(kBlock) void k_tick(uint8_t* __restrict__ bytes, TickOffsets t, uint32_t n,
                                                 const uint32_t* __restrict__ init, uint32_t init_step,
                                                 uint16_t* __restrict__ out, int mode, uint16_t* __restrict__ ip_ck,
                                                 uint16_t* __restrict__ tcp_ck, uint8_t* __restrict__ status,
                                                 const uint8_t* __restrict__ zpad, Done done) {
  const uint32_t g = threadIdx.x >> 4, lane = threadIdx.x & 15u;
  const uint32_t bsh = frame_shift(bytes);
  bytes -= bsh;
  // the wave's four groups' five bounds by scalar loads at a wave-uniform
  // index, in the kernel's first batch of argument loads (nothing they
  // depend on is loaded: the array is zero past n, an idle group's segment
  // is empty), then each group picks its pair
  const uint32_t w4 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * 4u;
  uint64_t o[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) o[k] = t.o[w4 + k];
  const uint32_t q = g & 3u;
  uint64_t s = o[0], e = o[1];
#pragma unroll
  for (uint32_t k = 1; k < 4; ++k)
    if (q == k) s = o[k], e = o[k + 1];
  const bool valid = g < n;
  s += bsh;
  e = valid ? e + bsh : s;
  const uint32_t gi = valid ? g : 0u;
  if constexpr (OP == 0) {
    const uint32_t i0 = init[gi * init_step];
    uint32_t ev = 0, od = 0;
    seg_sums<16, 8, true, 3>(bytes, s, e, lane, ev, od);
    const uint32_t tot = group_sum<16>(combine_roles(ev, od, uint32_t(s) & 1u));
    if (valid && lane == 15) out[g] = fold_value(i0 + tot);
  } else {
    const uint32_t* const zlast = reinterpret_cast<const uint32_t*>(zpad) + 7;
    ipv4_item<16, 8, true, 3>(bytes, s, e, g, valid, lane, mode, ip_ck, tcp_ck, status, zpad, zlast);
  }
  signal_done(done);
}

// ---------------------------------------------- resident tick server -----
// A one-block kernel that stays resident between ticks and takes each tick's
// job from a mailbox in coherent page-locked host memory (TickMailbox,
// icsum_launch.h) instead of being launched per tick: a tick then pays no
// launch (the ~3-5 us from the doorbell to the first wave), only the
// mailbox poll and the payload's PCIe reads.  Every descriptor word carries
// the job's sequence number in its high half, so one poll (wave 0: lane k
// reads word k, lane 63 the quit word) that finds the expected number in
// every word the job uses has read a complete descriptor, whatever order the
// host's stores landed in.  The job runs as k_tick's body (16-lane group per
// segment, starts / lengths from the descriptor), its results go to the
// job's page-locked result area, and `done` takes the sequence number with a
// system-scope release.  The server exits on the quit word, after idle_us
// without a job, or after kSrvMaxLife of 100 MHz ticks (the host relaunches
// it when a job finds it gone): every wave reaches an exit.
// Several blocks (ics_ctx::srv_blocks): block b serves mailbox b, with its
// own sequence numbers; a tick of n > 16 segments is split over mailboxes
// 0 .. ceil(n / 16) - 1 (w[kSrvPart]: the sub-job's first segment and the
// tick's n place its results), and every tick has a part in mailbox 0.  Block
// 0 alone decides to leave (quit word, idle, lifetime) and says so in its
// `state`; blocks b > 0 poll that word in place of the quit word and leave
// once they see it, so the grid leaves as a whole and the host relaunches
// only a grid that has fully left (no two blocks ever serve one mailbox).
constexpr uint64_t kSrvMaxLife = 100000000ull;  // 1 s of s_memrealtime

__global__ __launch_bounds__(kBlock) void k_tick_server(uint64_t* words, TickMailbox* mbs,
                                                        const uint8_t* __restrict__ zpad, uint32_t idle_us,
                                                        uint32_t pollers) {
  __shared__ uint32_t s_desc[64];
  __shared__ uint32_t s_cmd;  // 0 none yet, 1 a job, 2 exit
  TickMailbox* const mb = mbs + blockIdx.x;
  const uint64_t* const mw = words + kSrvWords * blockIdx.x;  // this block's descriptor words
  const bool lead = blockIdx.x == 0;
  const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t g = threadIdx.x >> 4, gl = threadIdx.x & 15u;
  const uint32_t* const zlast = reinterpret_cast<const uint32_t*>(zpad) + 7;
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint64_t t_job = t0;
  // the oldest job of this mailbox not done (the grid before this one has
  // left: its last `done` store is final)
  uint32_t expect = uint32_t(__hip_atomic_load(&mb->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) + 1u;
  // lane 63's poll word: the quit word (block 0) or block 0's exit word
  const uint64_t* const w63 = lead ? &words[kSrvQuit] : &words[kSrvExit];
  if (threadIdx.x == 0) s_cmd = 0u;
  __syncthreads();
  for (;;) {
    // waves 0 .. pollers - 1 poll, each on its own, started a fraction of a
    // PCIe round trip apart: a job posted at a random moment is seen by the
    // next poll to start, sooner with more pollers.  The first to see the
    // job, the quit word or the idle limit claims s_cmd (a job claimed
    // first wins over another wave's idle verdict); the rest stop polling.
    if (wv < pollers) {
      for (uint32_t k = 0; k < wv; ++k) __builtin_amdgcn_s_sleep(14);  // ~0.4 us each
      while (__hip_atomic_load(&s_cmd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) {
        const uint64_t word =
            __hip_atomic_load(lane == kSrvQuit ? w63 : &mw[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t pay = uint32_t(word), seq = uint32_t(word >> 32);
        const uint32_t w0 = __builtin_amdgcn_readlane(pay, 0), s0 = __builtin_amdgcn_readlane(seq, 0);
        const uint32_t nj = (w0 >> 8) & 0xffu, nw = kSrvHead + 2u * nj;  // the words this job uses
        const bool inits = (w0 >> 16) & 1u;
        const bool used = lane < nw || lane == kSrvPart || (inits && lane >= kSrvInit && lane < kSrvInit + nj);
        const bool fresh = !used || seq == expect;
        const bool job = s0 == expect && __all(fresh);
        const uint64_t q = __builtin_amdgcn_readlane(uint32_t(word | (word >> 32)), kSrvQuit);
        const bool quit = q != 0;
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        // blocks b > 0 leave with block 0 (their lifetime bound only a backstop)
        const bool idle = lead ? now - t_job > uint64_t(idle_us) * 100u || now - t0 > kSrvMaxLife
                               : now - t0 > 2 * kSrvMaxLife;
        if (job && !quit) s_desc[lane] = pay;  // (another poller may store the same words)
        if (job || quit || idle) {
          if (lane == 0) {
            uint32_t none = 0u;
            __hip_atomic_compare_exchange_strong(&s_cmd, &none, quit ? 2u : job ? 1u : 2u, __ATOMIC_RELAXED,
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    }
    __syncthreads();
    const uint32_t cmd = s_cmd;
    if (cmd == 2u) break;  // uniform
    // a resident kernel gets no launch-time cache invalidation: without this
    // system-scope acquire its loads of the reused staging slots would hit
    // the previous job's lines still held in L1 / L2
    // (the L2 holds such lines: without it, or with the CU's L1 alone
    // invalidated, the tests read the previous job's bytes;
    // profiles/r6_tick_server_inv.jsonl)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    // the job: checksum (op 0) or the fused IPv4 item (op 1, mode), n <= 16
    // segments at [bytes + s_j, + len_j), results into the page-locked area
    const uint32_t w0 = s_desc[0], op = w0 & 0xfu, mode = (w0 >> 4) & 0xfu, n = (w0 >> 8) & 0xffu;
    // the sub-job's segments are the tick's [first, first + n) of nt
    const uint32_t first = s_desc[kSrvPart] & 0xffu, nt = (s_desc[kSrvPart] >> 8) & 0xffu;
    uint8_t* bytes = reinterpret_cast<uint8_t*>(uint64_t(s_desc[1]) | (uint64_t(s_desc[2]) << 32));
    const uint32_t* init = reinterpret_cast<const uint32_t*>(uint64_t(s_desc[3]) | (uint64_t(s_desc[4]) << 32));
    uint8_t* res = reinterpret_cast<uint8_t*>(uint64_t(s_desc[5]) | (uint64_t(s_desc[6]) << 32));
    const uint32_t bsh = frame_shift(bytes);
    bytes -= bsh;
    const bool valid = g < n;
    const uint32_t gi = valid ? g : 0u;
    const uint64_t s = uint64_t(s_desc[kSrvHead + 2u * gi]) + bsh;
    const uint64_t e = valid ? s + s_desc[kSrvHead + 2u * gi + 1u] : s;
    // per-segment words (inits, message records) requested with the stream,
    // unconditionally (a load under a branch is waited for at its join,
    // ahead of the stream: one more PCIe round trip)
    const uint32_t* const iw = init ? init : reinterpret_cast<const uint32_t*>(zpad);
    if (op == 0u) {
      const uint32_t i0 = (w0 >> 16) & 1u ? s_desc[kSrvInit + gi] : 0u;
      uint32_t ev = 0, od = 0;
      seg_sums<16, 8, true, 3>(bytes, s, e, gl, ev, od);
      const uint32_t tot = group_sum<16>(combine_roles(ev, od, uint32_t(s) & 1u));
      if (valid && gl == 15) reinterpret_cast<uint16_t*>(res)[first + g] = uint16_t(fold_value(i0 + tot));
    } else if (op == 2u) {
      // wrap_tcp_in_ip (tcp_over_ip.cpp:69-88) as k_tcp_wrap with its headers
      // to an array: the payload after 40 bytes of header room (mode 0) or
      // the segment alone (mode 1); the record (ics_tcp_msg) at `init`
      const bool ok = valid && (mode == 1u || e - s >= 40);
      const uint64_t p0 = ok ? (mode == 1u ? s : s + 40) : e;
      const uint32_t* rec = iw + 7u * (first + gi);  // 28-byte records
      uint32_t r[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) r[k] = rec[k];
      uint32_t ev = 0, od = 0;
      seg_sums<16, 8, true, 3>(bytes, p0, e, gl, ev, od);
      const uint32_t tot = __shfl(group_sum<16>(combine_roles(ev, od, uint32_t(p0) & 1u)),
                                  int((threadIdx.x & 63u) | 15u), 64);  // to every lane of the group
      const u32x4 a{r[0], r[1], r[2], r[3]};
      uint32_t w[10], ipc, tcv;
      wrap_header(a, r[4], r[5], r[6] & 0xffffu, e - p0, tot, w, ipc, tcv);
      uint32_t wk = w[0];
#pragma unroll
      for (uint32_t k = 1; k < 10; ++k) wk = gl == k ? w[k] : wk;
      if (ok && gl < 10) reinterpret_cast<uint32_t*>(res)[10u * (first + g) + gl] = wk;
    } else {
      uint16_t* ip = reinterpret_cast<uint16_t*>(res);
      ipv4_item<16, 8, true, 3>(bytes, s, e, g, valid, gl, int(mode), ip + first, ip + nt + first,
                                res + 4u * nt + first, zpad, zlast);
    }
    // results out before `done` (signal_done's order): every wave's stores
    // retired, the block's barrier, one system-scope release
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      __hip_atomic_store(&mb->done, uint64_t(expect), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    ++expect;
    t_job = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) s_cmd = 0u;  // every wave read it at the barrier before the done store
    __syncthreads();  // s_desc / s_cmd are rewritten by the next poll
  }
  if (threadIdx.x == 0) {
    if (lead) __hip_atomic_store(&words[kSrvExit], uint64_t(1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&mb->state, uint64_t(kSrvExited), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

hipError_t launch_tick(const uint8_t* bytes, const uint64_t* offsets, uint32_t n, int op, const uint32_t* init,
                       uint16_t* out, int mode, uint16_t* ip_ck, uint16_t* tcp_ck, uint8_t* status,
                       const void* zero16, const Done& done, hipStream_t st) {
  if (n == 0 || n > kTickSegs || !bytes || !offsets) return hipErrorInvalidValue;
  TickOffsets t{};
  for (uint32_t j = 0; j <= n; ++j) t.o[j] = offsets[j];
  uint8_t* const b = const_cast<uint8_t*>(bytes);
  const SegWords w = seg_words(init, nullptr, zero16);
  const uint8_t* z = static_cast<const uint8_t*>(zero16);
  if (op == 0)
    hipLaunchKernelGGL(k_tick<0>, dim3(1), dim3(kBlock), 0, st, b, t, n, w.ip, w.is, out, 0, nullptr, nullptr,
                       nullptr, z, done);
  else if (mode >= 0 && mode <= 2)
    hipLaunchKernelGGL(k_tick<1>, dim3(1), dim3(kBlock), 0, st, b, t, n, w.ip, 0u, nullptr, mode, ip_ck, tcp_ck,
                       status, z, done);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_tick_server(uint64_t* words, TickMailbox* mbs, uint32_t blocks, const void* zero16,
                              uint32_t idle_us, uint32_t pollers, hipStream_t st) {
  if (pollers < 1 || pollers > kBlock / 64 || blocks < 1 || blocks > kSrvBlocksMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tick_server, dim3(blocks), dim3(kBlock), 0, st, words, mbs,
                     static_cast<const uint8_t*>(zero16), idle_us, pollers);
  return hipGetLastError();
}

}  // namespace icsum
