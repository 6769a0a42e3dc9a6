// icsum_route.cpp — the route table behind ics_route_table_* (include/icsum.h):
// Router::add_route / Router::match (src/router/router.cpp:15-24, :77-87)
// restated as a table of adds that is compiled, lazily, into the flat 16-8-7
// trie of icsum_route.h.  Plain C++: no HIP, no context, usable (and tested)
// on a machine without a GPU; the device path only takes the compiled image.
//
// Reference semantics kept (see the header): add stores under
// (L, rotr(prefix, 32 - L)), so a prefix with a bit below its top L bits has a
// key no addr >> (32 - L) can equal — the route is accepted and dead; match
// tries L = 31..0, so bit 0 of the address never counts and the longest live
// prefix wins; the last add of a (L, prefix) wins.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "icsum_route.h"

namespace icsum::detail {
// icsum_api.cpp's error reporting; absent (null) when this file is linked alone
int fail(int code, const char* fmt, ...) __attribute__((weak, format(printf, 2, 3)));
}  // namespace icsum::detail

namespace {

struct Route {
  uint32_t prefix, len, iface, next_hop;
  bool has_next_hop;
};

std::atomic<uint64_t> g_table_id{0}, g_table_gen{0};

#define ROUTE_FAIL(code, ...) (::icsum::detail::fail ? ::icsum::detail::fail((code), __VA_ARGS__) : (code))

bool live(const Route& r) {
  // the low 32 - L bits are what rotr moves to the top of the key
  return r.len == 0 ? r.prefix == 0 : (r.prefix & ((uint32_t(1) << (32 - r.len)) - 1)) == 0;
}

}  // namespace

struct ics_route_table {
  std::mutex mu;
  uint64_t id = 0, gen = 0;
  std::vector<Route> adds;  // in add order
  bool compiled = false;
  std::vector<uint32_t> image;  // trie words, then the route records
  ics_route_stats_t stats{};
};

namespace {

using icsum::detail::kRouteChild;
using icsum::detail::kRouteDirect;
using icsum::detail::kRouteL1Words;
using icsum::detail::kRouteL2Words;
using icsum::detail::kRouteL3Words;

// a new chunk of `words` words filled with `leaf`; its word index, or 0 when
// the image would reach 2^31 words
uint32_t new_chunk(std::vector<uint32_t>& w, uint64_t words, uint32_t leaf) {
  if (w.size() + words >= (uint64_t(1) << 31)) return 0;
  const uint32_t at = uint32_t(w.size());
  w.resize(w.size() + words, leaf);
  return at;
}

// Build order: live routes only, the last add per (L, prefix), increasing L —
// so a slot a longer route lands in holds the longest shorter route that
// covers it (leaf pushing), and a chunk made from a leaf starts filled with it.
int compile(ics_route_table* t) {
  if (t->compiled) return ICS_OK;
  try {
    ics_route_stats_t st{};
    st.routes_added = t->adds.size();
    std::vector<uint32_t> rec_of[32];  // per length: indices into `recs`, in first-add order
    std::unordered_map<uint64_t, uint32_t> seen;
    std::vector<Route> recs;
    for (const Route& r : t->adds) {
      if (!live(r)) {
        ++st.routes_dead;
        continue;
      }
      ++st.routes_live;
      const uint64_t key = uint64_t(r.len) << 32 | r.prefix;
      auto it = seen.find(key);
      if (it != seen.end()) {
        recs[it->second] = r;  // a later add replaces the earlier one
      } else {
        seen.emplace(key, uint32_t(recs.size()));
        rec_of[r.len].push_back(uint32_t(recs.size()));
        recs.push_back(r);
      }
    }
    st.route_records = recs.size();
    std::vector<uint32_t> w(kRouteL1Words, 0u);
    for (uint32_t L = 0; L < 32; ++L) {
      for (uint32_t k : rec_of[L]) {
        const uint32_t p = recs[k].prefix, leaf = k + 1;
        if (L <= 16) {  // no chunk exists yet: only shorter-or-equal routes are in
          const uint32_t a = p >> 16, cnt = uint32_t(1) << (16 - L);
          for (uint32_t j = 0; j < cnt; ++j) w[a + j] = leaf;
          continue;
        }
        uint32_t c2 = w[p >> 16];
        if (!(c2 & kRouteChild)) {
          const uint32_t at = new_chunk(w, kRouteL2Words, c2);
          if (!at) return ROUTE_FAIL(ICS_ERR_NOMEM, "route image would reach 2^31 words");
          ++st.l2_chunks;
          w[p >> 16] = c2 = at | kRouteChild;
        }
        const uint64_t b2 = c2 & ~kRouteChild;
        if (L <= 24) {  // no level-3 chunk exists yet
          const uint32_t a = (p >> 8) & 255u, cnt = uint32_t(1) << (24 - L);
          for (uint32_t j = 0; j < cnt; ++j) w[b2 + a + j] = leaf;
          continue;
        }
        uint32_t c3 = w[b2 + ((p >> 8) & 255u)];
        if (!(c3 & kRouteChild)) {
          const uint32_t at = new_chunk(w, kRouteL3Words, c3);
          if (!at) return ROUTE_FAIL(ICS_ERR_NOMEM, "route image would reach 2^31 words");
          ++st.l3_chunks;
          w[b2 + ((p >> 8) & 255u)] = c3 = at | kRouteChild;
        }
        const uint64_t b3 = c3 & ~kRouteChild;
        const uint32_t a = (p >> 1) & 127u, cnt = uint32_t(1) << (31 - L);
        for (uint32_t j = 0; j < cnt; ++j) w[b3 + a + j] = leaf;
      }
    }
    st.image_words = w.size();
    w.reserve(w.size() + 2 * recs.size());
    for (const Route& r : recs) {
      w.push_back(r.iface | (r.has_next_hop ? 0u : kRouteDirect));
      w.push_back(r.has_next_hop ? r.next_hop : 0u);
    }
    t->image.swap(w);
    t->stats = st;
    t->compiled = true;
  } catch (const std::bad_alloc&) {
    return ROUTE_FAIL(ICS_ERR_NOMEM, "route image allocation failed");
  }
  return ICS_OK;
}

void changed(ics_route_table* t) {
  t->compiled = false;
  t->gen = ++g_table_gen;
}

}  // namespace

namespace icsum::detail {

int route_image_acquire(ics_route_table* tbl, RouteImageView* view) {
  if (!tbl || !view) return ROUTE_FAIL(ICS_ERR_INVALID, "null route table");
  tbl->mu.lock();
  if (int rc = compile(tbl)) {
    tbl->mu.unlock();
    return rc;
  }
  view->id = tbl->id;
  view->gen = tbl->gen;
  view->words = tbl->image.data();
  view->nwords = tbl->stats.image_words;
  view->nrecs = uint32_t(tbl->stats.route_records);
  return ICS_OK;
}

void route_image_release(ics_route_table* tbl) { tbl->mu.unlock(); }

}  // namespace icsum::detail

extern "C" {

int ics_route_table_create(ics_route_table** out) {
  if (!out) return ROUTE_FAIL(ICS_ERR_INVALID, "null output pointer");
  *out = nullptr;
  ics_route_table* t = new (std::nothrow) ics_route_table();
  if (!t) return ROUTE_FAIL(ICS_ERR_NOMEM, "route table allocation failed");
  t->id = ++g_table_id;
  t->gen = ++g_table_gen;
  *out = t;
  return ICS_OK;
}

int ics_route_table_destroy(ics_route_table* tbl) {
  delete tbl;
  return ICS_OK;
}

int ics_route_table_add(ics_route_table* tbl, uint32_t prefix, uint32_t prefix_len, uint32_t iface,
                        int has_next_hop, uint32_t next_hop) {
  if (!tbl) return ROUTE_FAIL(ICS_ERR_INVALID, "null route table");
  if (prefix_len > 31)
    return ROUTE_FAIL(ICS_ERR_INVALID, "prefix length %u above 31 (32 is undefined behaviour in Router::add_route)",
                      prefix_len);
  if (iface >= 0x80000000u) return ROUTE_FAIL(ICS_ERR_INVALID, "interface %u not below 2^31", iface);
  std::lock_guard<std::mutex> lock(tbl->mu);
  try {
    tbl->adds.push_back(Route{prefix, prefix_len, iface, has_next_hop ? next_hop : 0u, has_next_hop != 0});
  } catch (const std::bad_alloc&) {
    return ROUTE_FAIL(ICS_ERR_NOMEM, "route table allocation failed");
  }
  changed(tbl);
  return ICS_OK;
}

int ics_route_table_clear(ics_route_table* tbl) {
  if (!tbl) return ROUTE_FAIL(ICS_ERR_INVALID, "null route table");
  std::lock_guard<std::mutex> lock(tbl->mu);
  tbl->adds.clear();
  changed(tbl);
  return ICS_OK;
}

int ics_route_table_match(ics_route_table* tbl, uint32_t addr, uint32_t* iface, uint32_t* next_hop) {
  if (!tbl) return ROUTE_FAIL(ICS_ERR_INVALID, "null route table");
  std::lock_guard<std::mutex> lock(tbl->mu);
  if (int rc = compile(tbl)) return rc;
  const uint32_t* w = tbl->image.data();
  const uint32_t leaf = icsum::detail::route_walk(w, addr);
  if (!leaf) {
    if (iface) *iface = ICS_NO_ROUTE;
    if (next_hop) *next_hop = 0;
    return 0;
  }
  const uint32_t* r = w + tbl->stats.image_words + 2 * uint64_t(leaf - 1);
  if (iface) *iface = r[0] & ~kRouteDirect;
  if (next_hop) *next_hop = (r[0] & kRouteDirect) ? addr : r[1];
  return 1;
}

int ics_route_table_stats(ics_route_table* tbl, ics_route_stats_t* stats) {
  if (!tbl || !stats) return ROUTE_FAIL(ICS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(tbl->mu);
  if (int rc = compile(tbl)) return rc;
  *stats = tbl->stats;
  return ICS_OK;
}

}  // extern "C"
