// icsum_kernels.hip — HIP kernels of the Internet-checksum engine, CDNA4 (gfx950).
//
// Every kernel is a memory-bound integer fold: HBM-read roofline, no MFMA.
//   k_checksum    a1-a4  InternetChecksum{init}.add(seg).value()  (checksum.h:17-41)
//                        or the unfolded sum_ for add() chains (checksum.h:44-59)
//   k_ipv4_tcp    a7/a8/a10/a11/a13 fused per raw datagram: header checksum,
//                        pseudo-header, TCP compute/verify, optional in-place patch
//                        (ipv4_header.cpp:9-123, tcp_segment.cpp:9-118, tcp_over_ip.cpp:69-88)
//   k_router_ttl  router.cpp:43-50 ttl-- + header recompute in place
// plus the synthetic-workload generators of icsum_workload.h.
//
// Work mapping: a group of LPS lanes (4..64, aligned inside the 64-lane wave)
// owns one segment; each lane streams 16-byte chunks with non-temporal
// dwordx4 loads (UNROLL in flight per step), accumulates with v_dot4_u32_u8,
// and the group reduces with cross-lane shuffles.  Segments are independent,
// so there is no inter-workgroup communication and no XCD dependence.

// One translation unit (the bounds word and the block stamps are shared by
// every family).  Each family's device functions, kernels and launchers:
//   icsum_common.h      block size, SegSrc / Work, block_order, signal_done, launch helpers
//   icsum_binning.h     k_bin_stats, k_bin_plan, k_bin_scatter
//   icsum_checksum.h    k_checksum, _small, _tiny, _twoclass, _dense, _bins, k_fold
//   icsum_ipv4.h        header fields, k_ipv4_tcp, k_ipv4_twoclass
//   icsum_batchv.h      k_checksum_batchv, k_ipv4_batchv
//   icsum_wrap.h        k_tcp_wrap, k_tcp_hdr
//   icsum_tick.h        k_tick, k_tick_server
//   icsum_route.h       the route image walk (Router::match), k_route_lookup
//   icsum_hdrpass.h     what the header-only passes share: rows_load / row_take, pair_hdr_load,
//                       hdr_parses / hop_rewrite, wave_store (no kernels; router, frame, unwrap include it)
//   icsum_router.h      k_router_ttl, k_router_hdrs (<true>: the route lookup fused)
//   icsum_frame.h       k_frame (<false>: recv_frame's classification, <true>: the hop over Ethernet frames)
//   icsum_unwrap.h      k_tcp_unwrap (message records behind the VERIFY launch)
//   icsum_span.h        k_span (tile launches)
//   icsum_scatter.h     k_copy_pieces (the receive streams' gather / scatter)
//   icsum_generators.h  the workload generators
// (icsum_device.h: arithmetic primitives; icsum_launch.h: the launchers' interface)
#include "icsum_common.h"
#include "icsum_binning.h"
#include "icsum_checksum.h"
#include "icsum_ipv4.h"
#include "icsum_batchv.h"
#include "icsum_wrap.h"
#include "icsum_tick.h"
#include "icsum_route.h"
#include "icsum_router.h"
#include "icsum_frame.h"
#include "icsum_unwrap.h"
#include "icsum_span.h"
#include "icsum_scatter.h"
#include "icsum_generators.h"

namespace icsum {

#ifdef ICSUM_BOUNDS_CHECK
__device__ BoundsState g_icsum_bounds;
#endif

void set_xcd_remap(uint32_t run_log2) { g_xcd_remap = run_log2 < 31 ? run_log2 : 31; }

bool bounds_checked_build() {
#ifdef ICSUM_BOUNDS_CHECK
  return true;
#else
  return false;
#endif
}

hipError_t bounds_take(hipStream_t st, uint32_t* flags, uint64_t* what) {
  *flags = 0;
  *what = 0;
#ifdef ICSUM_BOUNDS_CHECK
  BoundsState b{};
  if (hipError_t e = hipStreamSynchronize(st)) return e;
  if (hipError_t e = hipMemcpyFromSymbol(&b, HIP_SYMBOL(g_icsum_bounds), sizeof b)) return e;
  if (b.flags) {
    const BoundsState z{};
    if (hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_icsum_bounds), &z, sizeof z)) return e;
  }
  *flags = b.flags;
  *what = b.addr;
#else
  (void)st;
#endif
  return hipSuccess;
}

}  // namespace icsum
