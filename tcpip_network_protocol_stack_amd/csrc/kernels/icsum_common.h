// icsum_common.h — what every kernel family of icsum_kernels.hip shares: the
// block size, where a launch finds its segments (SegSrc / Work), the XCD block
// order, the zero-copy completion, and the host-side launch helpers (grid
// sizes, the geometry table, absent arrays, out_kind).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "icsum_device.h"
#include "icsum_launch.h"

namespace icsum {
namespace {

constexpr int kBlock = 256;

// segment i's bounds in the kernel's frame (sh = frame_shift of the batch's
// byte base, icsum_device.h)
__device__ __forceinline__ void seg_bounds(const uint64_t* __restrict__ offsets, uint64_t stride,
                                           uint64_t seg_len, uint64_t i, uint64_t& s,
                                           uint64_t& e, uint32_t sh) {
  if (offsets) {
    s = offsets[i];
    e = offsets[i + 1];
#ifdef ICSUM_BOUNDS_CHECK
    if (e < s) bounds_fail(kBoundsOffsets, i);  // offsets must be monotone
#endif
  } else {
    s = i * stride;
    e = s + seg_len;
  }
  s += sh;
  e += sh;
}

// k_bin_plan's plans (described at PlanCostTable, icsum_binning.h)
constexpr uint32_t kPlanWhole = 0, kPlanSplit = 1, kPlanWhole16 = 2, kPlanWholeSmall = 3;
static_assert(kPlanWhole == kPlanWholeBatch && kPlanSplit == kPlanSplitBins && kPlanWhole16 == kPlanWholeBatch16 &&
              kPlanWholeSmall == kPlanWholeBatchSmall, "plan ids shared with the host's plan cache");

// Where a launch finds its segments: fixed stride, packed offsets, or a
// length bin written by k_bin_segments (entries {start lo, start hi, length,
// segment index}; capacity n, so any index < n is a safe read).
struct SegSrc {
  const uint64_t* offsets;
  uint64_t stride, seg_len;
  const u32x4* list;     // bin launch: this bin's entries
  const uint32_t* meta;  // bin launch: the binning pass's sizes and plan
  int bin;
  uint32_t shift = 0;    // frame_shift of the byte base, set by the kernel (rebase)
};

// the kernel's frame of its byte base (icsum_device.h): bytes moved down to
// the 16-byte-aligned address, the shift recorded for src_decode
template <typename T>
__device__ __forceinline__ T* rebase(T* bytes, SegSrc& src) {
  src.shift = frame_shift(bytes);
  return bytes - src.shift;
}

// A launch's work, resolved once at kernel start: the bin's list (split plan)
// or, for the last bin's launch under the whole-batch plan, every segment by
// index.  Items are walked by a grid stride; the last bin's launch has one
// lane group per segment of the batch (no stride), bins 0..3 a capped grid.
struct Work {
  uint64_t items;
  const u32x4* list;  // null: segment i = item i
};

__device__ __forceinline__ Work resolve(const SegSrc& src, uint64_t n) {
  if (!src.list) return Work{n, nullptr};
  // selects, not branches, keep every path explicit
  const uint32_t plan = src.meta[kBinMetaPlan];
  const bool split = plan == kPlanSplit;
  const bool last = src.bin == kBins - 1;
  Work w;
  w.items = split ? uint64_t(src.meta[kBinMetaCount + src.bin]) : (last && plan == kPlanWhole ? n : 0);
  w.list = split ? src.list : nullptr;
  return w;
}

constexpr uint32_t kLongEntry = 0xFFFFFFFFu;  // entry length: >= 4 GiB, re-read the offsets

// Raw metadata of one work item (loads from clamped indices, so they are
// unconditional and never wait at a join).
struct ItemMeta {
  u32x4 ent;     // list entry
  uint64_t a, b;  // offsets[i], offsets[i + 1]
};

__device__ __forceinline__ ItemMeta src_fetch(const SegSrc& src, const Work& w, uint64_t gi, uint64_t n) {
  ItemMeta m{};
  const uint64_t c = gi < n ? gi : n - 1;  // list capacity n, offsets n + 1
  if (w.list) {
    m.ent = w.list[c];
  } else if (src.offsets) {
    m.a = src.offsets[c];
    m.b = src.offsets[c + 1];
  }
  return m;
}

// segment number, start and end of work item gi; an item past the end
// (gi >= items) gets seg = s = e = 0
__device__ __forceinline__ void src_decode(const SegSrc& src, const Work& w, uint64_t gi, const ItemMeta& m,
                                           uint64_t& seg, uint64_t& s, uint64_t& e) {
  seg = s = e = 0;
  if (gi >= w.items) return;
  if (w.list) {
    seg = m.ent.w;
    if (m.ent.z != kLongEntry) {
      s = uint64_t(m.ent.x) | (uint64_t(m.ent.y) << 32);
      e = s + m.ent.z;
    } else {
      seg_bounds(src.offsets, 0, 0, seg, s, e, 0u);
    }
  } else {
    seg = gi;
    if (src.offsets) {
      s = m.a;
      e = m.b;
#ifdef ICSUM_BOUNDS_CHECK
      if (e < s) bounds_fail(kBoundsOffsets, gi);  // offsets must be monotone
#endif
    } else {
      s = gi * src.stride;
      e = s + src.seg_len;
    }
  }
  s += src.shift;  // the kernel's frame (rebase)
  e += src.shift;
}

__device__ __forceinline__ void src_locate(const SegSrc& src, const Work& w, uint64_t gi, uint64_t n,
                                           uint64_t& seg, uint64_t& s, uint64_t& e) {
  src_decode(src, w, gi, src_fetch(src, w, gi, n), seg, s, e);
}

// XCD-aware block order.  Blocks b and b + 8 are observed to share an XCD
// (MI355X_MICROARCH.md §Workgroup dispatch: blocks are dealt round-robin over
// the 8 XCDs), so the hardware order gives every XCD every 8th block — each
// XCD's L2 and address translation see 8 disjoint pieces per run of blocks.
// Remapped, XCD label x = b % 8 takes runs of c consecutive logical blocks
// (c = min(run, grid / 8), powers of two): each XCD streams contiguous memory, neighbouring
// segments (whose shared boundary lines mode 3 keeps in L2) sit on one XCD,
// and the 8 runs still form one front of 8c blocks.  Blocks past the last
// whole 8c window keep their order (a bijection for any grid).  Measured,
// interleaved in one process on 5 boxes (profiles/r1_ab_xcd.jsonl):
//   NS 1 M x 1500 B     213.3 -> 208.5 us   (FETCH 1.5855 -> 1.5771 GB)
//   1 M x 9000 B       1307.0 -> 1255.5 us
//   8 M x 9000 B      10524.9 -> 10087.9 us
// (c = grid / 8, i.e. eight contiguous eighths, lost 1.8 % on the 75 GB batch).
// c is a power of two (run_log2 caps it), so the mapping is shifts and masks:
// short-lived blocks (small segments) pay a few scalar instructions, not an
// emulated integer division per block.
__device__ __forceinline__ uint32_t block_order(uint32_t run_log2) {
  const uint32_t nblk = gridDim.x, b = blockIdx.x;
  if (run_log2 == 0 || nblk < 16) return b;
  const uint32_t fl = 31u - uint32_t(__builtin_clz(nblk >> 3));  // floor(log2(nblk / 8))
  const uint32_t lc = fl < run_log2 ? fl : run_log2;              // c = 2^lc
  const uint32_t full = (nblk >> (lc + 3)) << (lc + 3);           // whole 8c windows
  if (b >= full) return b;
  const uint32_t k = b >> 3, x = b & 7u;
  return ((k >> lc) << (lc + 3)) + (x << lc) + (k & ((1u << lc) - 1u));
}

// End of a launch that completes a zero-copy host call (Done): every wave
// first waits for its own outstanding memory operations (s_waitcnt 0: on
// gfx9 stores count in vmcnt, so its result stores have left the CU — made
// explicit rather than relying on the barrier's workgroup-scope release to
// emit that wait), then the block's barrier orders them before lane 0, whose
// system-scope release (cumulative: one L2 write-back per block, not per
// wave) puts them where the host reads them before it takes a ticket; the
// block with the last ticket resets the ticket word and releases the
// completion value into the host word.  A one-block launch (a tick of up to
// 16 MTU datagrams) skips the ticket and releases the word at once: the
// agent-scope atomic behind the system-scope release cost 1.7-1.9 us of a
// 9-13 us call (profiles/r5_tick_latency_single_block_ab.jsonl).  A no-op
// (one uniform branch) for every device-path launch.  Every thread of the
// block must reach it: kernels call their body first.
__device__ __forceinline__ void signal_done(const Done& d) {
  if (d.flag == nullptr) return;
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
    if (gridDim.x == 1) {  // the only block (a tick of a few datagrams): no ticket to draw
      __hip_atomic_store(d.flag, d.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    const uint32_t t = __hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (t == gridDim.x - 1) {
      __hip_atomic_store(d.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(d.flag, d.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// HSA dispatch packets carry the grid size in work-items as a uint32, so
// element-wise kernels use a capped grid and stride over the rest.
#define ICS_GRID_STRIDE(i, n) \
  for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < (n); i += uint64_t(gridDim.x) * blockDim.x)

// The most 256-thread blocks one dispatch holds: HSA packets carry the grid
// in work-items as a uint32, so 2^24 blocks would be one work-item too many.
// The two-class launches (one block per 64 or 128 segments) refuse batches
// past it with hipErrorInvalidValue, and the dispatch falls back to a
// grid-stride launch (8-lane groups / the fused kernel).
constexpr uint64_t kMaxGridBlocks = (uint64_t(1) << 24) - 1;
constexpr uint64_t twoclass_blocks(uint64_t n, uint64_t spw) {  // 4 waves x spw segments per block
  return (n + (kBlock / 64) * spw - 1) / ((kBlock / 64) * spw);
}
static_assert(uint64_t(kBlock) * kMaxGridBlocks <= 0xFFFFFFFFull, "grid work-items fit a uint32");
// the boundary ADVICE r3 found: n in (2^31 - 128, 2^31] at 32 per wave (or
// (2^30 - 64, 2^30] at 16) needs 2^24 blocks and must be refused
static_assert(twoclass_blocks((uint64_t(1) << 31) - 127, 32) > kMaxGridBlocks &&
                  twoclass_blocks((uint64_t(1) << 31) - 128, 32) == kMaxGridBlocks &&
                  twoclass_blocks((uint64_t(1) << 30) - 63, 16) > kMaxGridBlocks &&
                  twoclass_blocks((uint64_t(1) << 30) - 64, 16) == kMaxGridBlocks,
              "two-class grids: the largest batches that still fit");

// element-wise grid: at most 64K blocks (16M work-items), grid-stride beyond
inline uint32_t ew_blocks(uint64_t n) {
  const uint64_t b = (n + kBlock - 1) / kBlock;
  return uint32_t(b == 0 ? 1 : (b < 65536 ? b : 65536));
}

inline uint32_t blocks_for(uint64_t groups, uint32_t groups_per_block, uint32_t max_blocks) {
  uint64_t b = (groups + groups_per_block - 1) / groups_per_block;
  if (b == 0) b = 1;
  // cap keeps blocks * 256 work-items far below the uint32 AQL grid limit;
  // the kernels grid-stride over the remaining segments
  const uint64_t cap = max_blocks ? max_blocks : (uint64_t(1) << 22);
  return uint32_t(b < cap ? b : cap);
}

uint32_t g_xcd_remap = 10;  // log2 of the XCD run length of block_order (1024 blocks); 0: hardware order

inline SegSrc src_of(const SegSpec& sp) {
  return SegSrc{sp.offsets, sp.stride, sp.seg_len, static_cast<const u32x4*>(sp.list), sp.meta, sp.bin};
}

// every instantiated (LPS, UNROLL, NT, MODE) of k_checksum, k_ipv4_tcp and
// k_tcp_wrap: exactly the shapes the dispatch can reach — pick_geometry's line
// grids, the last bin's 32/64-lane launch, the fused kernel's 4/8-lane shapes of
// short datagrams (ipv4_geometry), its one-lane shape for ACK-sized datagrams
// (mode 0, default-policy loads) and the 8-lane groups of ACK + MTU mixes
#define ICS_GEOMETRIES(X)                                                                     \
  X(1, 4, false, 0) X(4, 1, true, 2) X(4, 2, true, 2) X(8, 2, true, 2) X(8, 8, true, 3)      \
  X(16, 4, true, 3) X(16, 5, true, 3) X(16, 6, true, 3) X(16, 7, true, 3) X(16, 8, true, 3) \
  X(32, 8, true, 3) X(64, 8, true, 3)

// small-segment kernel instantiations (LPS, UNROLL, SEGS); Geometry::segs > 1
#define ICS_SMALL_GEOMETRIES(X) X(4, 1, 2) X(4, 2, 2) X(8, 2, 2)

// The match-and-call chains over the two tables, written once: f gets the
// matching entry's parameters as std::integral_constant values (usable as
// template arguments: launch_x_t<L(), U(), ...>); returns whether one matched.
template <int V>
using int_c = std::integral_constant<int, V>;

template <typename F>
bool for_geometry(Geometry g, F&& f) {
#define ICS_CASE(L, U, T, A)                                    \
  if (g.lps == L && g.unroll == U && g.nt == T && g.mode == A) \
    return f(int_c<L>{}, int_c<U>{}, std::bool_constant<T>{}, int_c<A>{}), true;
  ICS_GEOMETRIES(ICS_CASE)
#undef ICS_CASE
  return false;
}

template <typename F>
bool for_small_geometry(Geometry g, F&& f) {
#define ICS_SMALL(L, U, K) \
  if (g.lps == L && g.unroll == U && g.segs == K) return f(int_c<L>{}, int_c<U>{}, int_c<K>{}), true;
  ICS_SMALL_GEOMETRIES(ICS_SMALL)
#undef ICS_SMALL
  return false;
}

// f(OUT) with out_kind (0: u16 value(), 1: u32 raw sum) as a constant, and
// the same for a flag
template <typename F>
auto with_out(int out_kind, F&& f) {
  return out_kind == 0 ? f(int_c<0>{}) : f(int_c<1>{});
}
template <typename F>
auto with_flag(bool flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// The per-segment arrays of a checksum launch as the kernels take them: never
// null, an absent array replaced by the 16-byte zero buffer read with index
// step 0.
struct SegWords {
  const uint32_t* ip;
  uint32_t is;
  const uint8_t* op;
  uint32_t os;
};
inline SegWords seg_words(const uint32_t* init, const uint8_t* odd, const void* zero16) {
  return {init ? init : static_cast<const uint32_t*>(zero16), init ? 1u : 0u,
          odd ? odd : static_cast<const uint8_t*>(zero16), odd ? 1u : 0u};
}

}  // namespace
}  // namespace icsum
