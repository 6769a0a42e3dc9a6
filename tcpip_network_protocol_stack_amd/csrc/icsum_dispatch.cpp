// icsum_dispatch.cpp — device-buffer dispatch behind the C-ABI (icsum_api.cpp):
// which kernel and geometry runs a batch, the plan cache that remembers the
// device's view of an offsets batch's length mix, the binned launches, the
// device wrap's one- or two-pass choice and the multi-batch grouping.  Each
// single-batch path (checksum, fused IPv4, wrap) is one plan read
// (plan_lookup), one pure choice (choose_*: a Launch by value) and one issuer
// (issue_*: the launches, the re-plan behind them, ics_dispatch_info's
// fields).  All arithmetic happens in the HIP kernels
// (kernels/icsum_kernels.hip and its family headers).
#include <algorithm>
#include <string>
#include <vector>

#include "icsum_ctx.h"

namespace icsum::detail {

static_assert(icsum::kBvDense64 == ICS_BV_DENSE64 && icsum::kBvTiny == ICS_BV_TINY && icsum::kBvSmall == ICS_BV_SMALL &&
                  icsum::kBvLine16 == ICS_BV_LINE16 && icsum::kBvLine64 == ICS_BV_LINE64 &&
                  icsum::kBvLane1 == ICS_BV_LANE1,
              "multi-batch shapes are reported as ICS_BV_*");

// the geometries the dispatch names itself (the others come from pick_geometry)
constexpr icsum::Geometry kLine16x8{16, 8, true, 3, 1};  // the 16-lane line grid of MTU-sized segments
constexpr icsum::Geometry kLine8x8{8, 8, true, 3, 1};    // 8-lane groups
constexpr icsum::Geometry kLane1{1, 4, false, 0, 1};     // fused kernels: one lane per datagram, default-policy loads

// Segments per k_span wave: the forced value; with the cached plan's mean
// length (capped at 4095 by the plan), about ics_ctx::kSpanBytes of segments
// per span, 1..63 (a wave streams its span alone: spans of long segments
// leave the chip a few long-lived waves); without one, 63.  Measured
// (tools/ab_stream.py; profiles/r5n_ab_span_size.jsonl,
// r5o_ab_span_size_fine.jsonl; us back to back, S = 4 / 16 / 32 / 63): 1 M
// x 40..1040 B checksum 236.3 / 89.9 / 83.9 / 91.2, VERIFY 315.7 / 122.3 /
// 111.6 / 122.2; 1 M x 770 B checksum 250.4 / 129.1 / 118.4 / 123.1;
// 128 Ki of config 4's 64 B..64 KiB mix VERIFY 191.5 / 209.3 / 221.1 /
// 265.9 — flat from about 16 to 40 KiB per span.
uint32_t span_segs_for(const ics_ctx* ctx, uint32_t avg) {
  if (ctx->span_segs) return ctx->span_segs;
  if (avg == 0) return 63;
  return uint32_t(std::clamp<uint64_t>(ics_ctx::kSpanBytes / avg, 1, 63));
}

bool wrap_two_pass(const ics_ctx* ctx, bool headers_apart, uint64_t n) {
  return ctx->wrap_passes == 2 || (ctx->wrap_passes == 0 && headers_apart && n >= ics_ctx::kWrapTwoPassMin);
}

icsum::Geometry geometry_for(const ics_ctx* ctx, uint64_t avg_len) {
  icsum::Geometry g = icsum::pick_geometry(avg_len);
  if (ctx->force_lps) g = {ctx->force_lps, ctx->force_unroll ? ctx->force_unroll : g.unroll, g.nt, g.mode, 1};
  if (ctx->force_mode >= 0) g.mode = ctx->force_mode;
  if (ctx->force_segs > 0) g.segs = ctx->force_segs;
  if (!icsum::geometry_supported(g)) g.nt = !g.nt;  // a forced shape exists with one load policy
  if (!icsum::geometry_supported(g)) g = icsum::pick_geometry(avg_len);
  return g;
}

// the fused IPv4 kernel has no small-segment (multi-segment) variant: use the
// one-segment kernel of the same lane shape
icsum::Geometry ipv4_geometry(icsum::Geometry g) {
  g.segs = 1;
  if (g.mode == icsum::kModeTiny) g = {4, 1, true, 2, 1};  // the tiny kernel is checksum-only
  if (!icsum::geometry_supported(g)) g = kLine16x8;
  return g;
}

// Fixed-length datagrams of at most 1664 bytes on the 16 x 8 line grid: 7
// loads per lane still cover the span (<= 111 chunks with the line's head) in
// one pass, and the fused kernel drops from 82 to 76 VGPRs (5 -> 6 waves /
// SIMD): config 2 COMPUTE / PATCH / VERIFY 16.88 / 20.88 / 16.73 -> 16.74 /
// 20.68 / 16.58 us (profiles/r4_ab_ipv4_unroll7.jsonl).  The plain checksum
// keeps 8 (already 8 waves; 1 M x 1500 B 209.2 vs 211.2 us at 7).
icsum::Geometry ipv4_fixed_geometry(const ics_ctx* ctx, icsum::Geometry g, uint64_t len) {
  if (!forced_geometry(ctx) && g.lps == 16 && g.unroll == 8 && g.mode == 3 && len > 0 && len <= 1664) g.unroll = 7;
  return g;
}

namespace {

// average segment length for the geometry choice without reading d_offsets
uint64_t avg_len_hint(const uint64_t* offsets, uint64_t seg_len) {
  return offsets ? 65536 : seg_len;  // unknown mix: the long-segment geometry
}

int kernel_of(icsum::Geometry g) {
  return g.mode == icsum::kModeTiny ? ICS_K_TINY : g.segs > 1 ? ICS_K_SMALL : ICS_K_CHECKSUM;
}

// a1-a4 on device buffers.  An offsets batch of unknown length mix is split
// into length bins on the device (two passes over the offsets), and every bin
// runs with the geometry that suits its lengths; the bin lists live in
// stream-ordered scratch, so concurrent calls on different streams are safe.
//
// The plan cache (ics_ctx::plan_slot): a lookup finds the slot keyed by this
// batch's (offsets pointer, n) and trusts its word only when the word carries
// the slot's generation — i.e. it was written by a plan kernel this key's
// miss (or refresh) queued, and has landed.  The mix holds the shares
// k_bin_plan reported, in sixteenths: segments of <= 144 bytes, and bytes in
// segments over 1920 bytes.  A miss (re)keys the least recently used slot;
// req.want asks the issuer to queue the plan kernels (into req.dst, with
// req.gen) behind its launch: on a miss, on every kPlanRefresh-th hit, and
// every kPlanRefresh-th lookup of a key whose plan has not landed yet.  Each
// entry path reads the cache once, under its own conditions; all need an
// offsets batch of kSmallPlanMin..2^32 - 1 segments (the word holds n's low
// 32 bits).
struct PlanMix {
  uint32_t short16 = 0, long16 = 0, avg = 0;  // avg: mean segment length, bytes (capped at 4095)
};
struct PlanReq {
  bool want = false;
  uint64_t* dst = nullptr;  // device view of the slot's word
  uint32_t gen = 0;
};
struct PlanRead {
  bool hit = false;
  uint32_t plan = 0;  // icsum::kPlan* of a hit
  PlanMix mix;        // of a hit (zero on a miss)
  PlanReq req;
};
PlanRead plan_lookup(ics_ctx* ctx, const icsum::SegSpec& sp) {
  PlanRead r;
  if (!ctx->plan_host) return r;
  std::lock_guard<std::mutex> lock(ctx->plan_mu);
  int k = -1, lru = 0;
  for (int i = 0; i < ics_ctx::kPlanSlots; ++i) {
    const ics_ctx::PlanSlot& ps = ctx->plan_slot[i];
    if (ps.key == sp.offsets && ps.n == sp.n && ps.gen) k = i;
    if (ps.used < ctx->plan_slot[lru].used) lru = i;
  }
  if (k >= 0) {
    ics_ctx::PlanSlot& ps = ctx->plan_slot[k];
    ps.used = ++ctx->plan_clock;
    const uint64_t v = __atomic_load_n(ctx->plan_host + k, __ATOMIC_ACQUIRE);
    const bool again = ++ps.hits % ics_ctx::kPlanRefresh == 0;
    r.req = {again, ctx->plan_host_dev + k, ps.gen};
    r.hit = (v >> 56) == ps.gen && ((v >> 8) & 0xFFFFFFFFull) == (sp.n & 0xFFFFFFFFull);  // the word has landed
    if (r.hit) {
      r.plan = uint32_t(v & 0xfu);
      r.mix = {uint32_t(v >> 4) & 0xfu, uint32_t(v >> 40) & 0xfu, uint32_t(v >> 44) & 0xfffu};
    }
    (r.hit ? ctx->n_hits : ctx->n_misses).fetch_add(1, std::memory_order_relaxed);
    return r;
  }
  ics_ctx::PlanSlot& ps = ctx->plan_slot[lru];
  ctx->plan_gen = ctx->plan_gen % 254 + 1;  // 1..254: never the 0xFF of an unwritten word
  ps = {sp.offsets, sp.n, ctx->plan_gen, 0, ++ctx->plan_clock};
  __atomic_store_n(ctx->plan_host + lru, ~uint64_t(0), __ATOMIC_RELEASE);
  r.req = {true, ctx->plan_host_dev + lru, ps.gen};
  ctx->n_misses.fetch_add(1, std::memory_order_relaxed);
  return r;
}
bool plan_sized(const icsum::SegSpec& sp) {
  return sp.offsets && sp.n >= ics_ctx::kSmallPlanMin && sp.n <= 0xFFFFFFFFull;
}

constexpr size_t kMetaBytes = (icsum::kBinMetaBytesTotal + 255) & ~size_t(255);

// stats + plan kernels only (no lists) behind a launch: the plan for the next
// call with the same offsets lands in the slot plan_lookup named
int replan(ics_ctx* ctx, const icsum::SegSpec& sp, uint32_t lps, const PlanReq& req, hipStream_t st) {
  if (!req.want) return ICS_OK;
  Scratch meta(ctx, kMetaBytes, st);
  ICS_HIP(meta.error());
  ICS_HIP(icsum::launch_bin_plan(sp.offsets, sp.n, static_cast<uint32_t*>(meta.get()), lps, req.dst, req.gen, st));
  ctx->n_replans.fetch_add(1, std::memory_order_relaxed);
  return ICS_OK;
}

// What a chooser decided, by value.  The issuers turn it into the launches
// and, through note, into ics_dispatch_info's last_* fields.
struct Launch {
  int kernel = 0;             // ICS_K_*
  icsum::Geometry g{};        // the per-segment launch; of a two-class or dense launch, the launch
                              // that runs when that launcher refuses the batch (lps 0: none)
  int plan = -1;              // the cached plan to report (-1: none)
  uint32_t max_blocks = 0;    // grid cap of the per-segment launch (0: one lane group per segment)
  uint32_t span = 0;          // ICS_K_TILE: segments per wave
  int tile_op = 0;            // ICS_K_TILE: ICS_TILE_*
  int spw = 0;                // two-class launches: segments per wave
  uint32_t plan_lps = 64;     // the re-plan's last_lps: the last bin's lanes in the plan kernel's cost model
};
Launch tile_launch(uint32_t span, int op, int plan) { return {ICS_K_TILE, {}, plan, 0, span, op}; }
Launch two_class(int kernel, int spw, icsum::Geometry fallback, int plan) { return {kernel, fallback, plan, 0, 0, 0, spw}; }

void note(ics_ctx* ctx, const icsum::SegSpec& sp, const Launch& L) {
  switch (L.kernel) {
    case ICS_K_TILE: return report_launch(ctx, L.kernel, int(L.span), L.tile_op, L.plan);
    case ICS_K_TWOCLASS:
    case ICS_K_IPV4_TWOCLASS: return report_launch(ctx, L.kernel, 16, L.spw, L.plan);  // the long segments' lanes
    case ICS_K_DENSE: return report_launch(ctx, L.kernel, int(sp.seg_len / 16), ctx->dense_segs, L.plan);
    default: return report_launch(ctx, L.kernel, L.g.lps, L.g.unroll, L.plan);
  }
}

// a batch of many short segments with (almost) no bytes in long ones: from
// kShortMix16 sixteenths of <= 144-byte segments and under 1/16 of the bytes
// in segments over 1920 bytes, one launch beats the binned launches and
// 16-lane groups — first 8-lane groups (1 M datagrams, 50 % / 75 % 40-byte
// ACKs + 1500 B: 139.5 / 107.4 us vs 146.0 / 125.6 us AUTO;
// profiles/r2_csum_mix_sweep.jsonl), now the two-class launch (mix_launch)
bool short_mix(const PlanMix& m) { return m.short16 >= ics_ctx::kShortMix16 && m.long16 == 0; }

// The tile launch (k_span) for an offsets batch whose device-reported mix
// favours it: from kTileMin segments, a mean length of at most kTileMaxAvg
// bytes (variable lengths leave per-segment lane groups idle), or — for the
// wraps, which have no length binning — a sixteenth or more of the bytes in
// segments over 1920 bytes; the fused IPv4 kernel on every mix but the
// short-heavy ones (choose_ipv4).  Short-heavy mixes keep the two-class
// launches (checked first by the callers), MTU-sized means the 16-lane line
// grid.  tools/ab_stream.py, profiles/r5l_ab_span_vs_per_segment.jsonl,
// r5m_ab_c4.jsonl, r5p_ab_span_thresholds.jsonl (us back to back,
// per-segment vs span): checksum 40..1040 B 256 Ki / 1 M 35.7 / 27.0 and
// 286.7 / 89.3, 770 B 1 M 153.0 / 122.8, MTU 1 M 212.2 / 236.8, 64 Ki 11.1 /
// 11.3; VERIFY 40..1040 B 64 Ki / 1 M 16.1 / 11.9 and 204.9 / 123.5, MTU
// 256 Ki / 1 M 70.4 / 61.3 and 264.6 / 237.6, 128 Ki of config 4's mix
// 233.5 / 192.3; headers-apart wrap 40..1040 B 64 Ki / 1 M 11.7 / 9.8 and
// 137.4 / 103.4, MTU 1 M 244.8 / 265.2; in-place wrap 40..1040 B 1 M 156.9 /
// 156.3, 770 B 1 M 193.2 / 207.2, config 4's mix 265.6 / 230.6.
// The plain checksum keeps the per-segment launches up to kTileMinChecksum
// (64 Ki 40..1040 B: 11.1 us per segment vs 11.3 us span above); VERIFY and
// the headers-apart wrap already win at 64 Ki (16.1 / 11.9, 11.7 / 9.8 us).
bool tile_wins(const ics_ctx* ctx, const PlanMix& m, uint64_t n, bool fused) {
  if (ctx->tile == 0 || n < (fused ? ics_ctx::kTileMin : ics_ctx::kTileMinChecksum)) return false;
  return m.avg <= ics_ctx::kTileMaxAvg || (fused && m.long16 >= 4);
}

// a short-heavy mix's single launch: the two-class launch (ACK-sized segments
// one per lane, the rest 16 lanes each; block lists since round 3), 32
// segments per wave from 3/4 short segments up and 16 below (round 2, the
// per-wave version: fewer long segments per wave, shorter-lived waves).  2 M x 40 / 1460 B: 8-lane groups 279.5, two-class 64 / 32 / 16 per
// wave 255.7 / 234.9 / 231.1 us; raw-datagram mixes (git 7692616:tools/ab_ipv4_mix.py
// plain rows, 64 / 32 / 16): 7/8 ACKs 43.5 / 42.2 / 54.5, 3/4 74.8 / 68.5 /
// 74.5, 1/2 132.4 / 122.5 / 119.0, 7/16 145.0 / 139.3 / 131.9 us
// (profiles/r2_twoclass_spw*.jsonl).  Batches past the two-class grid's
// limit run 8-lane groups.  It reports no plan.
Launch mix_launch(const PlanMix& mix) { return two_class(ICS_K_TWOCLASS, mix.short16 >= 12 ? 32 : 16, kLine8x8, -1); }

// the small-segment plan's single launch: one lane per segment for ACK-sized
// means (icsum::kTinyMaxAvg), else 4-lane groups with 2 segments in flight
icsum::Geometry small_plan_geometry(const PlanMix& m) {
  return m.avg <= icsum::kTinyMaxAvg ? icsum::Geometry{1, 4, false, icsum::kModeTiny, 1}
                                     : icsum::Geometry{4, 2, true, 2, 2};
}

// ---- checksum (a1-a4).  parity: the call carries a parity array (no dense kernel)
Launch choose_checksum(const ics_ctx* ctx, const icsum::SegSpec& sp, bool parity, bool binned, const PlanRead& pr) {
  if (sp.offsets && ctx->twoclass)  // test hook: the two-class launch on every offsets batch
    return two_class(ICS_K_TWOCLASS, ctx->twoclass, {}, -1);
  if (sp.offsets && ctx->tile == 1)  // test hook: the tile launch on every offsets batch
    return tile_launch(span_segs_for(ctx, 0), ICS_TILE_CHECKSUM, -1);
  const bool wholeS = pr.hit && pr.plan == icsum::kPlanWholeBatchSmall;
  const bool mix8 = pr.hit && !wholeS && short_mix(pr.mix);
  if (!binned) {
    if (mix8) return mix_launch(pr.mix);
    icsum::Geometry g = geometry_for(ctx, avg_len_hint(sp.offsets, sp.seg_len));
    // dense fixed-stride batch of short segments (config 3): the flat-array kernel
    if (!parity && ctx->dense_segs > 0 && !forced_geometry(ctx) && icsum::dense_supported(sp)) return {ICS_K_DENSE, g};
    // an offsets batch below the binning threshold: one launch, its geometry
    // from the plan the device reported for this batch last time (16-lane
    // groups for MTU-sized mixes, the small-segment body for short ones);
    // on a miss the unknown-mix geometry, and the plan kernels run behind
    // the launch for the next call (git 7692616:tools/ab_small_offsets.py)
    if (pr.hit && pr.plan == icsum::kPlanWholeBatch16) g = kLine16x8;
    if (wholeS) g = small_plan_geometry(pr.mix);
    return {kernel_of(g), g, pr.hit ? int(pr.plan) : -1};
  }
  // the whole-batch plan's launch geometry: one lane group per segment of the
  // batch; above 1 M segments 32-lane groups halve the waves an empty last bin
  // costs to dispatch
  icsum::Geometry g_last = icsum::bin_geometry(icsum::kBins - 1);
  const uint32_t lps = ctx->last_bin_lps ? ctx->last_bin_lps : (sp.n > (uint64_t(1) << 20) ? 32u : 64u);
  if (lps == 32) g_last = {32, 8, true, 3, 1};
  // the binning passes and the bin launches (issue_binned), under the forced plan if any
  Launch L{ICS_K_BINNED, g_last, ctx->bin_plan, ctx->last_bin_blocks};
  if (pr.hit && !mix8 && !wholeS && tile_wins(ctx, pr.mix, sp.n, false)) {
    L = tile_launch(span_segs_for(ctx, pr.mix.avg), ICS_TILE_CHECKSUM, int(pr.plan));
  } else if (mix8) {
    L = mix_launch(pr.mix);
  } else if (pr.hit && pr.plan != icsum::kPlanSplitBins) {
    // the whole-batch plan the device chose for this batch last time, as
    // its single launch: the last bin's geometry (whole), 16-lane groups
    // (whole16) or the small-segment body (wholeS) over every segment; a
    // short-heavy mix with no long segments (received traffic: ACKs + MTU
    // data) runs the two-class launch whatever the plan (mix_launch)
    const icsum::Geometry g_hit = pr.plan == icsum::kPlanWholeBatch16 ? kLine16x8
                                  : wholeS                           ? small_plan_geometry(pr.mix)
                                                                     : g_last;
    L = {kernel_of(g_hit), g_hit, int(pr.plan), pr.plan == icsum::kPlanWholeBatch ? ctx->last_bin_blocks : 0};
  }
  L.plan_lps = lps;
  return L;
}

// The binned launches: a hit with the split plan that neither tiles nor is
// short-heavy comes here too, and hands its re-plan request to the plan
// kernel of the binning passes
int issue_binned(ics_ctx* ctx, const icsum::SegSpec& sp, const uint32_t* d_init, const uint8_t* d_odd, void* d_out,
                 int out_kind, const Launch& L, const PlanReq& req, hipStream_t st) {
  Scratch ws(ctx, kMetaBytes + sp.n * 16 * icsum::kBins, st);
  ICS_HIP(ws.error());
  uint32_t* meta = static_cast<uint32_t*>(ws.get());
  void* list = static_cast<uint8_t*>(ws.get()) + kMetaBytes;
  // the binning passes; the plan kernel also reports into the plan cache's
  // slot when this call's lookup asked for a plan
  hipError_t e = icsum::launch_bin_segments(sp.offsets, sp.n, list, meta, ctx->bin_plan, L.plan_lps,
                                            req.want ? req.dst : nullptr, req.gen, st);
  // bins 0..3: one launch, a capped grid striding over each bin; the last
  // bin: one lane group per segment of the batch (it takes the whole batch
  // under the whole-batch plans)
  if (e == hipSuccess)
    e = icsum::launch_checksum_bins(icsum::bin_spec(sp, list, meta, 0), d_init, d_odd, d_out, out_kind,
                                    ctx->bin_blocks, st);
  if (e == hipSuccess)
    e = icsum::launch_checksum(icsum::bin_spec(sp, list, meta, icsum::kBins - 1), d_init, d_odd, d_out, out_kind,
                               L.g, L.max_blocks, st);
  ICS_HIP(e);
  if (req.want) ctx->n_replans.fetch_add(1, std::memory_order_relaxed);
  note(ctx, sp, L);
  return ICS_OK;
}

int issue_checksum(ics_ctx* ctx, const icsum::SegSpec& sp, const uint32_t* d_init, const uint8_t* d_odd, void* d_out,
                   int out_kind, Launch L, const PlanReq& req, hipStream_t st) {
  if (L.kernel == ICS_K_BINNED) return issue_binned(ctx, sp, d_init, d_odd, d_out, out_kind, L, req, st);
  hipError_t e;
  if (L.kernel == ICS_K_TWOCLASS)
    e = icsum::launch_checksum_twoclass(sp, d_init, d_odd, d_out, out_kind, L.spw, ctx->twoclass_remap, st, ctx->twoclass_lds);
  else if (L.kernel == ICS_K_DENSE)
    e = icsum::launch_checksum_dense(sp, d_init, d_out, out_kind, ctx->dense_segs, st);
  else if (L.kernel == ICS_K_TILE)
    e = icsum::launch_tile_checksum(sp, d_init, d_odd, d_out, out_kind, L.span, st, ctx->span_blocks);
  else
    e = icsum::launch_checksum(sp, d_init, d_odd, d_out, out_kind, L.g, L.max_blocks, st);
  // a batch past the two-class grid's limit, a (seg_len, segs) the dense
  // kernel is not instantiated for: the per-segment launch
  if (e == hipErrorInvalidValue && (L.kernel == ICS_K_TWOCLASS || L.kernel == ICS_K_DENSE) && L.g.lps) {
    L.kernel = kernel_of(L.g);
    e = icsum::launch_checksum(sp, d_init, d_odd, d_out, out_kind, L.g, 0, st);
  }
  ICS_HIP(e);
  note(ctx, sp, L);
  // re-plan behind it: a batch whose mix changed under the same pointer
  // and size is re-binned from the next call on
  return replan(ctx, sp, L.plan_lps, req, st);
}

// ---- fused IPv4 + TCP (b1-b4)
Launch choose_ipv4(const ics_ctx* ctx, const icsum::SegSpec& sp, const PlanRead& pr) {
  // an offsets batch of raw datagrams gives no length hint; datagrams are at
  // most 64 KiB and mostly MTU-sized, and the 16-lane line grid is the best
  // measured geometry for both 1500- and 9000-byte datagrams (64 Ki x 1500 B:
  // 18.3 us vs 48.8 us with the 64-lane default; git 7692616:tools/ab_ipv4_offsets.py)
  // ACK-sized datagrams (a fixed length <= kTinyMaxAvg, or a cached plan
  // whose mean is) run one lane per datagram with default-policy loads
  // (neighbours share lines): 1 M x 40 B VERIFY 30.3 -> 10.6 us (git 7692616:tools/ab_ipv4_mix.py, AB_LANE1)
  const icsum::Geometry base = geometry_for(ctx, sp.offsets ? 1500 : sp.seg_len);
  icsum::Geometry g = base.mode == icsum::kModeTiny ? kLane1 : ipv4_geometry(base);
  if (!sp.offsets) g = ipv4_fixed_geometry(ctx, g, sp.seg_len);
  // a receive batch of mostly short datagrams (pure ACKs: 40 bytes) leaves
  // most of a 16-lane group idle: from 16 Ki datagrams up the geometry
  // follows the plan the device reported for the same offsets buffer last
  // time (4-lane groups when it was the small-segment plan, 8-lane groups
  // from 5/16 of <= 144-byte datagrams, 16 x 4 below that), the plan
  // kernels running behind the first and every 64th launch (DESIGN.md §4,
  // git 7692616:tools/ab_ipv4_mix.py, profiles/r2_ipv4_mix_sweep.jsonl)
  const PlanMix& mix = pr.mix;
  const bool wholeS = pr.hit && pr.plan == icsum::kPlanWholeBatchSmall;
  if (wholeS && mix.avg <= icsum::kTinyMaxAvg)
    g = kLane1;
  else if (wholeS)
    g = ipv4_geometry({4, 2, true, 2, 1});
  else if (pr.hit && mix.short16 >= ics_ctx::kIpv4ShortMix16 && mix.long16 == 0)
    g = ipv4_geometry(kLine8x8);  // ACK + MTU mixes past the two-class grid's limit
  else if (pr.hit)
    g = ipv4_geometry({16, 4, true, 3, 1});  // MTU + a few ACKs: shorter unroll, 1-4 % (1 M datagrams)
  // the two-class launch (block lists, ics_ctx::kIpv4TwoClass16 for the
  // crossover against 16 x 4 groups; round 2's per-wave version beat the
  // 8-lane groups from 5/16 ACKs up, git 7692616:tools/ab_ipv4_mix.py)
  const bool two = pr.hit && !wholeS && mix.short16 >= ics_ctx::kIpv4TwoClass16 && mix.long16 == 0;
  // ACK-heavy mixes: 128 datagrams per block, so the block's one short
  // pass carries more of them (3/4 ACKs 78.4 -> 75.4 us, mix_probe blk32)
  const int spw = mix.short16 >= ics_ctx::kIpv4TwoClassWide16 ? 32 : 16;
  const int plan = pr.hit ? int(pr.plan) : -1;
  const bool tile = pr.hit && !two && !wholeS && ctx->tile != 0 && sp.n >= ics_ctx::kTileMin;
  if (sp.offsets && (ctx->tile == 1 || tile))  // the test hook, or the cached mix favours the tile launch
    return tile_launch(span_segs_for(ctx, pr.hit ? mix.avg : 0u), ICS_TILE_IPV4, plan);
  if (sp.offsets && ctx->twoclass) return two_class(ICS_K_IPV4_TWOCLASS, ctx->twoclass, g, plan);  // test hook
  return two ? two_class(ICS_K_IPV4_TWOCLASS, spw, g, plan) : Launch{ICS_K_IPV4, g, plan};
}

int issue_ipv4(ics_ctx* ctx, const icsum::SegSpec& sp, int mode, uint16_t* d_ip_ck, uint16_t* d_tcp_ck,
               uint8_t* d_status, Launch L, const PlanReq& req, hipStream_t st) {
  hipError_t e = hipErrorInvalidValue;
  if (L.kernel == ICS_K_TILE)
    e = icsum::launch_tile_ipv4(sp, mode, d_ip_ck, d_tcp_ck, d_status, L.span, st, ctx->span_blocks);
  else if (L.kernel == ICS_K_IPV4_TWOCLASS)
    e = icsum::launch_ipv4_twoclass(sp, mode, d_ip_ck, d_tcp_ck, d_status, L.spw, ctx->twoclass_remap, st, ctx->twoclass_lds);
  if (e == hipErrorInvalidValue && L.kernel != ICS_K_TILE) {  // no two-class launch, or past its grid's limit
    L.kernel = ICS_K_IPV4;
    e = icsum::launch_ipv4_tcp(sp, mode, d_ip_ck, d_tcp_ck, d_status, L.g, 0, st);
  }
  ICS_HIP(e);
  note(ctx, sp, L);
  return replan(ctx, sp, L.plan_lps, req, st);
}

// ---- the device wrap (c1)
// The device wrap's geometry: one lane per datagram for ACK-sized batches (a
// fixed length, or a cached small plan with a mean <= kTinyMaxAvg: 1 M pure
// ACKs in place 78.3 -> 36.6 us, 40-56 B 119.0 -> 47.4 us,
// git 7692616:tools/ab_wrap_ack.py), else the fused kernel's geometry for the length
// hint.  The plan kernels run behind the launch as plan_lookup asks (the
// wrap's transmit buffer keeps its own cache slot: a stack's receive-side
// verify in between does not evict it).
Launch choose_wrap(const ics_ctx* ctx, const icsum::SegSpec& sp, bool headers_apart, bool payload_only, uint64_t hint,
                   const PlanRead& pr) {
  const icsum::Geometry base = geometry_for(ctx, sp.offsets ? hint : sp.seg_len);
  icsum::Geometry g = base.mode == icsum::kModeTiny ? kLane1 : ipv4_geometry(base);
  const bool wholeS = pr.hit && pr.plan == icsum::kPlanWholeBatchSmall;
  if (wholeS && pr.mix.avg <= icsum::kTinyMaxAvg) g = kLane1;
  const int plan = pr.hit ? int(pr.plan) : -1;
  // the tile launch: the test hook; headers apart when the cached mix favours
  // it; in place only for long-segment mixes (its header stores cost the
  // same scattered write per datagram either way, and the per-segment wrap
  // is faster on short ones: 40..1040 B, 256 Ki: 40.3 / 44.7 us; config-4 mix
  // 499.3 / 464.2 us, git 7692616:tools/ab_dispatch.py).  Headers apart, the receive-side
  // mix of empty and MTU payloads tiles too (256 Ki / 1 M: 48.8 / 40.5 and
  // 169.3 / 150.8 us), payloads nearly all empty (pure ACKs) do not (1 M:
  // 24.2 / 41.0 us; profiles/r4_ab_dispatch_tile.jsonl)
  const PlanMix& mix = pr.mix;
  const bool tile_pick = pr.hit && !wholeS &&
                         (payload_only ? mix.short16 < ics_ctx::kTileApartShort16 && tile_wins(ctx, mix, sp.n, true)
                                       : !short_mix(mix) && ctx->tile != 0 && sp.n >= ics_ctx::kTileMin &&
                                             mix.long16 >= 4);
  if (sp.offsets && (ctx->tile == 1 || tile_pick))  // the wrap (in place or headers apart) as a tile launch
    return tile_launch(span_segs_for(ctx, pr.hit ? mix.avg : 0u), headers_apart ? ICS_TILE_WRAP_APART : ICS_TILE_WRAP, plan);
  // two passes (payload sums into n words of scratch, then the header launch) or one (ics_ctx::wrap_passes)
  return {wrap_two_pass(ctx, headers_apart, sp.n) ? ICS_K_WRAP_2PASS : ICS_K_WRAP, g, plan};
}

int issue_wrap(ics_ctx* ctx, const icsum::SegSpec& sp, const ics_tcp_msg* msgs, uint32_t* hdr_out, uint16_t* d_ip_ck,
               uint16_t* d_tcp_ck, bool payload_only, const Launch& L, const PlanReq& req, hipStream_t st) {
  const icsum::TcpMsg* m = reinterpret_cast<const icsum::TcpMsg*>(msgs);
  if (L.kernel == ICS_K_TILE) {
    ICS_HIP(icsum::launch_tile_wrap(sp, m, hdr_out, d_ip_ck, d_tcp_ck, L.span, st, ctx->span_blocks));
  } else if (L.kernel == ICS_K_WRAP) {
    ICS_HIP(icsum::launch_tcp_wrap(sp, m, hdr_out, d_ip_ck, d_tcp_ck, payload_only, nullptr, L.g, 0, st));
  } else {  // the scratch lease ends before the re-plan takes its own
    Scratch sums(ctx, sp.n * 4, st);
    ICS_HIP(sums.error());
    ICS_HIP(icsum::launch_tcp_wrap(sp, m, hdr_out, d_ip_ck, d_tcp_ck, payload_only, static_cast<uint32_t*>(sums.get()),
                                   L.g, 0, st));
  }
  note(ctx, sp, L);
  return replan(ctx, sp, L.plan_lps, req, st);
}

}  // namespace

int checksum_device(ics_ctx* ctx, const icsum::SegSpec& sp, const uint32_t* d_init, const uint8_t* d_odd,
                    void* d_out, int out_kind, hipStream_t st) {
  const bool hooked = sp.offsets && (ctx->twoclass || ctx->tile == 1);  // choose_checksum's first two lines
  const bool binned = sp.offsets && sp.n <= 0xFFFFFFFFull &&
                      (ctx->bin == 1 || (ctx->bin < 0 && sp.n >= ctx->bin_min && !forced_geometry(ctx)));
  // the plan cache serves the binned path, and below the binning threshold
  // unforced batches of a plan's size
  const bool planned = !hooked && ctx->bin < 0 && ctx->bin_plan < 0 && ctx->plan_host &&
                       (binned || (!forced_geometry(ctx) && plan_sized(sp)));
  const PlanRead pr = planned ? plan_lookup(ctx, sp) : PlanRead{};
  const Launch L = choose_checksum(ctx, sp, d_odd != nullptr, binned, pr);
  return issue_checksum(ctx, sp, d_init, d_odd, d_out, out_kind, L, pr.req, st);
}

int ipv4_device(ics_ctx* ctx, const icsum::SegSpec& sp, int mode, uint16_t* d_ip_ck, uint16_t* d_tcp_ck,
                uint8_t* d_status, hipStream_t st) {
  const bool planned = plan_sized(sp) && !forced_geometry(ctx) && !ctx->twoclass;
  const PlanRead pr = planned ? plan_lookup(ctx, sp) : PlanRead{};
  return issue_ipv4(ctx, sp, mode, d_ip_ck, d_tcp_ck, d_status, choose_ipv4(ctx, sp, pr), pr.req, st);
}

int wrap_device(ics_ctx* ctx, const icsum::SegSpec& sp, const ics_tcp_msg* d_msgs, uint32_t* hdr_out,
                uint16_t* d_ip_ck, uint16_t* d_tcp_ck, bool payload_only, uint64_t hint, hipStream_t st) {
  const PlanRead pr = plan_sized(sp) && !forced_geometry(ctx) ? plan_lookup(ctx, sp) : PlanRead{};
  const Launch L = choose_wrap(ctx, sp, hdr_out != nullptr, payload_only, hint, pr);
  return issue_wrap(ctx, sp, d_msgs, hdr_out, d_ip_ck, d_tcp_ck, payload_only, L, pr.req, st);
}

// k_copy_pieces over a piece list in device memory (ics_copy_pieces, ics_rx_stream_receive_batch).
int copy_pieces_device(ics_ctx* ctx, const void* d_src, uint64_t src_bytes, void* d_dst, uint64_t dst_bytes,
                       const void* d_pieces, uint64_t m, hipStream_t st) {
  ICS_HIP(icsum::launch_copy_pieces(static_cast<const uint8_t*>(d_src), src_bytes, static_cast<uint8_t*>(d_dst),
                                    uint32_t(dst_bytes), d_pieces, m, st));
  report_launch(ctx, ICS_K_COPY_PIECES);
  return ICS_OK;
}

// The VERIFY dispatch exactly as ics_ipv4_tcp_batch runs it (same plan cache
// slot, same choice), then one more launch on the stream for the records.
int unwrap_device(ics_ctx* ctx, const icsum::SegSpec& sp, ics_tcp_rx* d_recs, uint8_t* d_status, hipStream_t st) {
  std::unique_ptr<Scratch> lease;  // without d_status: held until both launches are enqueued
  if (!d_status) {
    {
      std::lock_guard<std::mutex> lock(ctx->unwrap_status.mu);
      if (!ctx->unwrap_status.ev) ICS_HIP(hipEventCreateWithFlags(&ctx->unwrap_status.ev, hipEventDisableTiming));
    }
    lease = std::make_unique<Scratch>(ctx->unwrap_status, sp.n, st);
    ICS_HIP(lease->error());
    d_status = static_cast<uint8_t*>(lease->get());
  }
  if (int rc = ipv4_device(ctx, sp, ICS_MODE_VERIFY, nullptr, nullptr, d_status, st)) return rc;
  ICS_HIP(icsum::launch_tcp_unwrap(sp, d_status, reinterpret_cast<uint32_t*>(d_recs), st));
  report_launch(ctx, ICS_K_UNWRAP);
  return ICS_OK;
}

int router_device(ics_ctx* ctx, const icsum::SegSpec& sp, uint32_t* d_hdrs, uint8_t* d_status, hipStream_t st) {
  if (d_hdrs) {
    ICS_HIP(icsum::launch_router_hdrs(sp, d_hdrs, d_status, st));
    report_launch(ctx, ICS_K_ROUTER_HDRS);
  } else {
    ICS_HIP(icsum::launch_router_ttl(sp, d_status, st));
    report_launch(ctx, ICS_K_ROUTER);
  }
  return ICS_OK;
}

namespace {
// Group the batches of a multi-batch call by kernel shape and issue one
// launch per group of up to kMaxBatchv (whose grids together stay below the
// dispatch's work-item limit); a batch too large for that runs alone through
// the single-batch path.
template <typename D, typename ClassFn, typename LaunchFn, typename AloneFn>
int run_batchv(ics_ctx* ctx, const D* b, uint32_t k, ClassFn cls_of, LaunchFn launch, AloneFn alone) {
  constexpr uint64_t kMaxBlocks = (uint64_t(1) << 24) - 1;
  std::vector<int> cls(k);
  for (uint32_t j = 0; j < k; ++j) cls[j] = b[j].n ? cls_of(b[j]) : -1;
  int last_cls = -1;
  for (int c = 0; c <= icsum::kBvLane1; ++c) {
    D group[icsum::kMaxBatchv];
    int m = 0;
    uint64_t blocks = 0;
    auto flush = [&]() -> int {
      if (m == 0) return ICS_OK;
      ICS_HIP(launch(group, m, c));
      last_cls = c;
      m = 0;
      blocks = 0;
      return ICS_OK;
    };
    for (uint32_t j = 0; j < k; ++j) {
      if (cls[j] != c) continue;
      const uint64_t nb = icsum::batchv_blocks(c, b[j].n);
      if (nb > kMaxBlocks / 4) {  // a large batch: a launch of its own, its usual path
        if (int rc = alone(b[j])) return rc;
        continue;
      }
      if (m == icsum::kMaxBatchv || blocks + nb > kMaxBlocks)
        if (int rc = flush()) return rc;
      group[m++] = b[j];
      blocks += nb;
    }
    if (int rc = flush()) return rc;
  }
  if (last_cls >= 0) report_launch(ctx, ICS_K_BATCHV, last_cls, int(k));
  return ICS_OK;
}
}  // namespace

int checksum_batchv_device(ics_ctx* ctx, const ics_seg_batch* batches, uint32_t k, hipStream_t st) {
  std::vector<icsum::BvSeg> b(k);
  for (uint32_t j = 0; j < k; ++j)
    b[j] = {static_cast<const uint8_t*>(batches[j].bytes), batches[j].offsets, batches[j].stride, batches[j].seg_len,
            batches[j].n, batches[j].init, batches[j].out, 0};
  auto cls_of = [&](const icsum::BvSeg& x) -> int {
    const icsum::SegSpec sp{x.bytes, x.offsets, x.stride, x.seg_len, x.n, ctx->d_zero};
    if (!x.offsets && x.seg_len == 64 && icsum::dense_supported(sp)) return icsum::kBvDense64;
    const icsum::Geometry g = icsum::pick_geometry(avg_len_hint(x.offsets, x.seg_len));
    if (g.mode == icsum::kModeTiny) return icsum::kBvTiny;
    if (g.segs > 1) return icsum::kBvSmall;
    return g.lps >= 32 ? icsum::kBvLine64 : icsum::kBvLine16;
  };
  auto launch = [&](const icsum::BvSeg* g, int m, int c) {
    return icsum::launch_checksum_batchv(g, m, c, ctx->d_zero, st);
  };
  auto alone = [&](const icsum::BvSeg& x) {
    const icsum::SegSpec sp{x.bytes, x.offsets, x.stride, x.seg_len, x.n, ctx->d_zero};
    return checksum_device(ctx, sp, x.init, nullptr, x.out, 0, st);
  };
  return run_batchv(ctx, b.data(), k, cls_of, launch, alone);
}

int ipv4_batchv_device(ics_ctx* ctx, const ics_dgram_batch* batches, uint32_t k, int mode, hipStream_t st) {
  std::vector<icsum::BvDgram> b(k);
  for (uint32_t j = 0; j < k; ++j)
    b[j] = {static_cast<uint8_t*>(batches[j].dgrams), batches[j].offsets, batches[j].stride, batches[j].dgram_len,
            batches[j].n, batches[j].ip_ck, batches[j].tcp_ck, batches[j].status};
  // the single call's unplanned choice: one lane per ACK-sized fixed-length
  // datagram, 64-lane groups past 3.5 KB, 16-lane line grids otherwise (and
  // for every offsets batch: mostly MTU-sized datagrams)
  auto cls_of = [&](const icsum::BvDgram& x) -> int {
    if (x.offsets) return icsum::kBvLine16;
    const icsum::Geometry g = icsum::pick_geometry(x.dlen);
    if (g.mode == icsum::kModeTiny) return icsum::kBvLane1;
    return g.lps >= 32 ? icsum::kBvLine64 : icsum::kBvLine16;
  };
  auto launch = [&](const icsum::BvDgram* g, int m, int c) {
    return icsum::launch_ipv4_batchv(g, m, c, mode, ctx->d_zero, st);
  };
  auto alone = [&](const icsum::BvDgram& x) {
    const icsum::SegSpec sp{x.dgrams, x.offsets, x.stride, x.dlen, x.n, ctx->d_zero};
    return ipv4_device(ctx, sp, mode, x.ip_ck, x.tcp_ck, x.status, st);
  };
  return run_batchv(ctx, b.data(), k, cls_of, launch, alone);
}

// ICSUM_FORCE (test hook): "key=value,key=value" forcing
// one kernel shape or dispatch decision so parity tests reach every
// instantiation.  An unknown key fails ics_create (a mistyped hook must not
// silently test the default path).
int apply_force(ics_ctx* ctx, const char* spec) {
  if (!spec || !*spec) return ICS_OK;
  std::string all(spec);
  size_t pos = 0;
  while (pos <= all.size()) {
    const size_t end = std::min(all.find(',', pos), all.size());
    const std::string item = all.substr(pos, end - pos);
    pos = end + 1;
    if (item.empty()) continue;
    const size_t eq = item.find('=');
    if (eq == std::string::npos) return fail(ICS_ERR_INVALID, "ICSUM_FORCE: '%s' is not key=value", item.c_str());
    const std::string k = item.substr(0, eq);
    char* tail = nullptr;
    const long long v = std::strtoll(item.c_str() + eq + 1, &tail, 0);
    if (!tail || *tail) return fail(ICS_ERR_INVALID, "ICSUM_FORCE: bad value in '%s'", item.c_str());
    if (k == "lps") ctx->force_lps = int(v);
    else if (k == "unroll") ctx->force_unroll = int(v);
    else if (k == "mode") ctx->force_mode = int(v);
    else if (k == "segs") ctx->force_segs = int(v);
    else if (k == "bin") ctx->bin = int(v);
    else if (k == "bin_min") ctx->bin_min = uint64_t(v);
    else if (k == "bin_plan") ctx->bin_plan = v >= 0 && v <= 3 ? int(v) : -1;
    else if (k == "bin_blocks") ctx->bin_blocks = uint32_t(std::max<long long>(v, 1));
    else if (k == "last_bin_lps") ctx->last_bin_lps = uint32_t(v);
    else if (k == "last_bin_blocks") ctx->last_bin_blocks = uint32_t(v);
    else if (k == "dense_segs") ctx->dense_segs = int(v);
    else if (k == "twoclass" && (v == 0 || v == 8 || v == 16 || v == 32)) ctx->twoclass = int(v);
    else if (k == "wrap_passes" && v >= 0 && v <= 2) ctx->wrap_passes = uint32_t(v);
    else if (k == "xcd_remap") icsum::set_xcd_remap(uint32_t(v));
    else if (k == "span_segs" && v >= 0 && v <= 63) ctx->span_segs = uint32_t(v);
    else if (k == "span_blocks" && v >= 0 && v <= 0xFFFFFF) ctx->span_blocks = uint32_t(v);
    else if (k == "tick_inline" && (v == 0 || v == 1)) ctx->tick_inline = int(v);
    else if (k == "slot_prio" && v >= -8 && v <= 8) ctx->slot_prio = int(v);
    else if (k == "tick_server" && v >= 0 && v <= 10000000) ctx->srv_idle_us = uint32_t(v);
    else if (k == "srv_pollers" && v >= 1 && v <= 4) ctx->srv_pollers = uint32_t(v);
    else if (k == "srv_blocks" && v >= 1 && v <= int64_t(icsum::kSrvBlocksMax)) ctx->srv_blocks = uint32_t(v);
    else if (k == "srv_vram" && (v == 0 || v == 1)) ctx->srv_vram = int(v);
    else if (k == "twoclass_remap" && v >= 0 && v <= 30) ctx->twoclass_remap = uint32_t(v);
    else if (k == "twoclass_lds" && v >= 0 && v <= 65536) ctx->twoclass_lds = uint32_t(v);
    else if (k == "zero_copy_max" && v >= 0) ctx->zero_copy_max = uint64_t(v);
    else if (k == "poison_ticket" && v > 0 && v <= 0xFFFFFFFFll) ctx->poison_ticket = uint32_t(v);
    else if (k == "tile" && v >= -1 && v <= 1) ctx->tile = int(v);
    else return fail(ICS_ERR_INVALID, "ICSUM_FORCE: unknown or out-of-range '%s'", item.c_str());
  }
  return ICS_OK;
}

}  // namespace icsum::detail
