// icsum_images.cpp — the route and neighbour tables' compiled images on the
// device (ics_ctx::route_slot / neigh_slot): which slot holds an image, its
// upload when the table changed, and the launches that read them
// (ics_route_lookup_batch, ics_router_route_*, ics_frame_recv_batch,
// ics_router_frames).
#include <algorithm>

#include "icsum_ctx.h"
#include "icsum_neigh.h"
#include "icsum_route.h"

namespace icsum::detail {

namespace {
// the table stays locked (its image valid) until the image is on the device
template <typename Table, void (*Release)(Table*)>
struct ImageLock {
  Table* tbl = nullptr;
  ~ImageLock() {
    if (tbl) Release(tbl);
  }
};

// The slot of `slots` that holds image (id, gen), uploaded on `st` when it is
// not there yet: the slot with that id, else the least recently used (an
// empty one first).  The caller holds ctx->route_mu and the table's lock (the
// host image `words` stays valid until the upload has landed).
int image_slot(ics_ctx* ctx, ics_ctx::RouteSlot (&slots)[ics_ctx::kRouteSlots], uint64_t id, uint64_t gen,
               const uint32_t* words, size_t need, uint64_t a, uint32_t b, hipStream_t st,
               ics_ctx::RouteSlot** out) {
  ics_ctx::RouteSlot* slot = nullptr;
  for (auto& s : slots)
    if (s.id == id) slot = &s;
  if (!slot) {
    slot = &slots[0];
    for (auto& s : slots)
      if (s.used < slot->used) slot = &s;
  }
  if (slot->id != id || slot->gen != gen) {
    slot->id = 0;  // not trusted until the upload has landed
    // launches on any stream may still read it: every stream's last one is behind its pair's event
    for (auto& r : slot->readers) ICS_HIP(hipEventSynchronize(r.ev));
    if (need > slot->cap) {
      const size_t cap = (std::max(need, 2 * slot->cap) + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
      void* p = nullptr;
      ICS_HIP(hipMalloc(&p, cap));
      if (slot->d) ctx->route_retired.push_back(slot->d);
      slot->d = static_cast<uint32_t*>(p);
      slot->cap = cap;
    }
    ICS_HIP(hipMemcpyAsync(slot->d, words, need, hipMemcpyHostToDevice, st));
    ICS_HIP(hipStreamSynchronize(st));  // the table's host image is released by the caller
    slot->id = id;
    slot->gen = gen;
    slot->nwords = a;
    slot->nrecs = b;
  }
  slot->used = ++ctx->route_clock;
  *out = slot;
  return ICS_OK;
}

int route_slot_for(ics_ctx* ctx, ics_route_table* tbl, hipStream_t st, ics_ctx::RouteSlot** out) {
  RouteImageView v;
  if (int rc = route_image_acquire(tbl, &v)) return rc;
  ImageLock<ics_route_table, route_image_release> held{tbl};
  return image_slot(ctx, ctx->route_slot, v.id, v.gen, v.words, (size_t(v.nwords) + 2 * size_t(v.nrecs)) * 4,
                    v.nwords, v.nrecs, st, out);
}

int neigh_slot_for(ics_ctx* ctx, ics_neigh_table* tbl, hipStream_t st, ics_ctx::RouteSlot** out) {
  NeighImageView v;
  if (int rc = neigh_image_acquire(tbl, &v)) return rc;
  ImageLock<ics_neigh_table, neigh_image_release> held{tbl};
  return image_slot(ctx, ctx->neigh_slot, v.id, v.gen, v.words, (size_t(v.nif) + size_t(v.nslots)) * 16, v.nif,
                    v.nslots, st, out);
}

// The launch that read the slot is behind the event of its stream's pair, or
// nothing may replace the image under it.  A stream new to the slot takes over
// a pair whose event has completed, else a new pair; no reader waits for
// another.
void slot_launched(ics_ctx::RouteSlot* slot, hipStream_t st) {
  ics_ctx::RouteSlot::Reader* r = nullptr;
  for (auto& x : slot->readers)
    if (x.st == st) r = &x;
  if (!r)
    for (auto& x : slot->readers)
      if (hipEventQuery(x.ev) == hipSuccess) {
        r = &x;
        break;
      }
  if (!r) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess) {
      slot->readers.push_back({st, ev});
      r = &slot->readers.back();
    }
  }
  if (r && hipEventRecord(r->ev, st) == hipSuccess) {
    r->st = st;
    return;
  }
  (void)hipStreamSynchronize(st);  // no event behind this launch: it is not in flight any more instead
}
}  // namespace

int route_device(ics_ctx* ctx, ics_route_table* tbl, const icsum::SegSpec* sp, const uint32_t* d_addrs, uint64_t n,
                 uint32_t* d_hdrs, uint8_t* d_status, uint32_t* d_iface, uint32_t* d_next_hop, hipStream_t st) {
  std::lock_guard<std::mutex> lock(ctx->route_mu);
  ics_ctx::RouteSlot* slot = nullptr;
  if (int rc = route_slot_for(ctx, tbl, st, &slot)) return rc;
  const icsum::RouteImg img{slot->d, slot->nwords, slot->nrecs};
  if (!sp) {
    ICS_HIP(icsum::launch_route_lookup(d_addrs, n, img, d_iface, d_next_hop, st));
    report_launch(ctx, ICS_K_ROUTE_LOOKUP);
  } else {
    ICS_HIP(icsum::launch_router_route(*sp, img, d_hdrs, d_status, d_iface, d_next_hop, st));
    report_launch(ctx, d_hdrs ? ICS_K_ROUTER_ROUTE_HDRS : ICS_K_ROUTER_ROUTE);
  }
  slot_launched(slot, st);
  return ICS_OK;
}

int frames_device(ics_ctx* ctx, ics_route_table* routes, ics_neigh_table* neigh, const icsum::SegSpec& sp,
                  uint32_t in_iface, const uint32_t* d_in_iface, uint32_t* d_hdrs, uint8_t* d_status,
                  uint32_t* d_iface, uint32_t* d_next_hop, hipStream_t st) {
  std::lock_guard<std::mutex> lock(ctx->route_mu);
  ics_ctx::RouteSlot *rs = nullptr, *ns = nullptr;
  if (routes)
    if (int rc = route_slot_for(ctx, routes, st, &rs)) return rc;
  if (int rc = neigh_slot_for(ctx, neigh, st, &ns)) return rc;
  const icsum::RouteImg rimg = rs ? icsum::RouteImg{rs->d, rs->nwords, rs->nrecs} : icsum::RouteImg{};
  const icsum::NeighImg nimg{ns->d, uint32_t(ns->nwords), ns->nrecs};
  ICS_HIP(icsum::launch_frames(sp, rimg, nimg, in_iface, d_in_iface, routes ? d_hdrs : nullptr, d_status, d_iface,
                               d_next_hop, st));
  report_launch(ctx, routes ? ICS_K_ROUTER_FRAMES : ICS_K_FRAME_RECV);
  if (rs) slot_launched(rs, st);
  slot_launched(ns, st);
  return ICS_OK;
}

void free_routes(ics_ctx* ctx) {
  for (auto* slots : {&ctx->route_slot, &ctx->neigh_slot})
    for (auto& s : *slots) {
      for (auto& r : s.readers) {
        (void)hipEventSynchronize(r.ev);
        (void)hipEventDestroy(r.ev);
      }
      if (s.d) (void)hipFree(s.d);
      s = {};
    }
  for (void* p : ctx->route_retired) (void)hipFree(p);
  ctx->route_retired.clear();
}

}  // namespace icsum::detail
