// icsum_neigh.cpp — the neighbour table behind ics_neigh_table_* (include/icsum.h):
// the control half of NetworkInterface (src/network_interface/network_interface.cpp:
// the constructor's addresses, arp_addr_table_, arp_requests_, tick, and the
// ARP branches of recv_frame / send_datagram) restated per interface, compiled
// lazily into the identity array + open-addressed table of icsum_neigh.h.
// Plain C++: no HIP, no context, usable (and tested) on a machine without a
// GPU; the device path only takes the compiled image.
//
// Reference semantics kept (see the header): per-interface cache, the two
// address destination filter, ARP parse = 28 bytes and supported(), learn from
// every ARP that parses, release on REPLY only, strict expiry comparisons, the
// request timer a wrapping uint32_t.  The queue of waiting datagrams is the
// caller's.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

#include "icsum_neigh.h"

namespace icsum::detail {
// icsum_api.cpp's error reporting; absent (null) when this file is linked alone
int fail(int code, const char* fmt, ...) __attribute__((weak, format(printf, 2, 3)));
}  // namespace icsum::detail

namespace {

#define NEIGH_FAIL(code, ...) (::icsum::detail::fail ? ::icsum::detail::fail((code), __VA_ARGS__) : (code))

using icsum::detail::kNeighConfigured;
using icsum::detail::kNeighMaxIface;
using icsum::detail::kNeighUsed;

constexpr uint64_t kMapDeadline = 30000;  // rto_map_
constexpr uint32_t kReqDeadline = 5000;   // rto_arp_

struct Mapping {
  uint8_t mac[6];
  uint64_t timer;  // size_t timer_
};

struct Iface {
  bool set = false;
  uint8_t mac[6] = {};
  uint32_t ip = 0;
  std::unordered_map<uint32_t, Mapping> map;   // arp_addr_table_
  std::unordered_map<uint32_t, uint32_t> req;  // arp_requests_
};

std::atomic<uint64_t> g_table_id{0}, g_table_gen{0};

uint32_t mac_lo(const uint8_t* m) { return uint32_t(m[0]) | uint32_t(m[1]) << 8 | uint32_t(m[2]) << 16 | uint32_t(m[3]) << 24; }
uint32_t mac_hi(const uint8_t* m) { return uint32_t(m[4]) | uint32_t(m[5]) << 8; }
uint32_t be16(const uint8_t* p) { return uint32_t(p[0]) << 8 | p[1]; }
uint32_t be32(const uint8_t* p) { return uint32_t(p[0]) << 24 | uint32_t(p[1]) << 16 | uint32_t(p[2]) << 8 | p[3]; }
void put_be32(uint8_t* p, uint32_t v) {
  p[0] = uint8_t(v >> 24);
  p[1] = uint8_t(v >> 16);
  p[2] = uint8_t(v >> 8);
  p[3] = uint8_t(v);
}

// make_frame(TYPE_ARP, serialize(make_arp_mesg(opcode, target_ip, target_ether)), dst)
void arp_frame(uint8_t* f, const Iface& me, uint32_t opcode, uint32_t target_ip, const uint8_t* target_mac) {
  std::memset(f, 0, 42);
  if (target_mac) std::memcpy(f, target_mac, 6);
  else std::memset(f, 0xff, 6);  // ETHERNET_BROADCAST
  std::memcpy(f + 6, me.mac, 6);
  f[12] = 0x08, f[13] = 0x06;
  f[14] = 0x00, f[15] = 0x01;  // TYPE_ETHERNET
  f[16] = 0x08, f[17] = 0x00;
  f[18] = 6, f[19] = 4;
  f[20] = uint8_t(opcode >> 8), f[21] = uint8_t(opcode);
  std::memcpy(f + 22, me.mac, 6);
  put_be32(f + 28, me.ip);
  if (target_mac) std::memcpy(f + 32, target_mac, 6);
  put_be32(f + 38, target_ip);
}

// IPv4Header::parse on `len` payload bytes (ipv4_header.cpp:9-59): twenty
// bytes present, version 4, hlen >= 5, and the checksum of the re-serialized
// header (cksum 0, the reserved flag bit dropped, no options) as given
bool ipv4_parses(const uint8_t* p, size_t len) {
  if (len < 20 || (p[0] >> 4) != 4 || (p[0] & 0x0f) < 5) return false;
  uint32_t s = 0;
  for (int k = 0; k < 20; k += 2) {
    uint32_t w = be16(p + k);
    if (k == 6) w &= 0x7fffu;
    if (k == 10) w = 0;
    s += w;
  }
  s = (s >> 16) + (s & 0xffffu);
  s = (s >> 16) + (s & 0xffffu);
  return uint32_t(~s & 0xffffu) == be16(p + 10);
}

}  // namespace

struct ics_neigh_table {
  std::mutex mu;
  uint64_t id = 0, gen = 0;
  std::vector<Iface> ifaces;  // indexed by interface number
  uint64_t mappings = 0;
  bool compiled = false;
  std::vector<uint32_t> image;
  uint32_t nslots = 0;
};

namespace {

void changed(ics_neigh_table* t) {
  t->compiled = false;
  t->gen = ++g_table_gen;
}

int compile(ics_neigh_table* t) {
  if (t->compiled) return ICS_OK;
  try {
    uint64_t nslots = 4;
    while (nslots < 2 * t->mappings) nslots <<= 1;
    if (nslots >= (uint64_t(1) << 28)) return NEIGH_FAIL(ICS_ERR_NOMEM, "neighbour image would reach 2^28 slots");
    const uint64_t nif = t->ifaces.size();
    std::vector<uint32_t> w(4 * nif + 4 * nslots, 0u);
    uint32_t* slots = w.data() + 4 * nif;
    const uint32_t mask = uint32_t(nslots) - 1;
    for (uint64_t f = 0; f < nif; ++f) {
      const Iface& it = t->ifaces[f];
      if (it.set) {
        w[4 * f] = mac_lo(it.mac);
        w[4 * f + 1] = mac_hi(it.mac) | kNeighConfigured;
        w[4 * f + 2] = it.ip;
      }
      for (const auto& kv : it.map) {
        uint32_t at = icsum::detail::neigh_hash(uint32_t(f), kv.first) & mask;
        while (slots[4 * uint64_t(at) + 1] != 0u) at = (at + 1) & mask;  // load <= 1/2: a free slot exists
        uint32_t* s = slots + 4 * uint64_t(at);
        s[0] = kv.first;
        s[1] = uint32_t(f) | kNeighUsed;
        s[2] = mac_lo(kv.second.mac);
        s[3] = mac_hi(kv.second.mac);
      }
    }
    t->image.swap(w);
    t->nslots = uint32_t(nslots);
    t->compiled = true;
  } catch (const std::bad_alloc&) {
    return NEIGH_FAIL(ICS_ERR_NOMEM, "neighbour image allocation failed");
  }
  return ICS_OK;
}

// the interface's entry, grown on demand; null when allocation fails
Iface* iface_at(ics_neigh_table* t, uint32_t iface) {
  try {
    if (iface >= t->ifaces.size()) {
      t->ifaces.resize(size_t(iface) + 1);
      changed(t);  // the identity array grew
    }
  } catch (const std::bad_alloc&) {
    return nullptr;
  }
  return &t->ifaces[iface];
}

int learn_locked(ics_neigh_table* t, uint32_t iface, uint32_t ip, const uint8_t* mac) {
  Iface* it = iface_at(t, iface);
  if (!it) return NEIGH_FAIL(ICS_ERR_NOMEM, "neighbour table allocation failed");
  try {
    auto found = it->map.find(ip);
    if (found == it->map.end()) {
      Mapping m{};
      std::memcpy(m.mac, mac, 6);
      it->map.emplace(ip, m);
      ++t->mappings;
      changed(t);
    } else {
      if (std::memcmp(found->second.mac, mac, 6) != 0) {
        std::memcpy(found->second.mac, mac, 6);
        changed(t);
      }
      found->second.timer = 0;  // insert_or_assign(AddrMapping(mac)): a new timer
    }
  } catch (const std::bad_alloc&) {
    return NEIGH_FAIL(ICS_ERR_NOMEM, "neighbour table allocation failed");
  }
  return ICS_OK;
}

void tick_one(ics_neigh_table* t, Iface& it, uint64_t ms) {
  for (auto e = it.map.begin(); e != it.map.end();) {
    e->second.timer += ms;
    if (e->second.timer > kMapDeadline) {
      e = it.map.erase(e);
      --t->mappings;
      changed(t);
    } else {
      ++e;
    }
  }
  for (auto e = it.req.begin(); e != it.req.end();) {
    e->second += uint32_t(ms);  // uint32_t += size_t, as the reference's
    if (e->second > kReqDeadline) e = it.req.erase(e);
    else ++e;
  }
}

}  // namespace

namespace icsum::detail {

int neigh_image_acquire(ics_neigh_table* tbl, NeighImageView* view) {
  if (!tbl || !view) return NEIGH_FAIL(ICS_ERR_INVALID, "null neighbour table");
  tbl->mu.lock();
  if (int rc = compile(tbl)) {
    tbl->mu.unlock();
    return rc;
  }
  view->id = tbl->id;
  view->gen = tbl->gen;
  view->words = tbl->image.data();
  view->nif = uint32_t(tbl->ifaces.size());
  view->nslots = tbl->nslots;
  return ICS_OK;
}

void neigh_image_release(ics_neigh_table* tbl) { tbl->mu.unlock(); }

}  // namespace icsum::detail

extern "C" {

int ics_neigh_table_create(ics_neigh_table** out) {
  if (!out) return NEIGH_FAIL(ICS_ERR_INVALID, "null output pointer");
  *out = nullptr;
  ics_neigh_table* t = new (std::nothrow) ics_neigh_table();
  if (!t) return NEIGH_FAIL(ICS_ERR_NOMEM, "neighbour table allocation failed");
  t->id = ++g_table_id;
  t->gen = ++g_table_gen;
  *out = t;
  return ICS_OK;
}

int ics_neigh_table_destroy(ics_neigh_table* tbl) {
  delete tbl;
  return ICS_OK;
}

int ics_neigh_table_set_iface(ics_neigh_table* tbl, uint32_t iface, const uint8_t mac[6], uint32_t ip) {
  if (!tbl || !mac) return NEIGH_FAIL(ICS_ERR_INVALID, "null argument");
  if (iface >= kNeighMaxIface) return NEIGH_FAIL(ICS_ERR_INVALID, "interface %u not below 65536", iface);
  std::lock_guard<std::mutex> lock(tbl->mu);
  Iface* it = iface_at(tbl, iface);
  if (!it) return NEIGH_FAIL(ICS_ERR_NOMEM, "neighbour table allocation failed");
  if (!it->set || std::memcmp(it->mac, mac, 6) != 0 || it->ip != ip) changed(tbl);
  it->set = true;
  std::memcpy(it->mac, mac, 6);
  it->ip = ip;
  return ICS_OK;
}

int ics_neigh_table_learn(ics_neigh_table* tbl, uint32_t iface, uint32_t ip, const uint8_t mac[6]) {
  if (!tbl || !mac) return NEIGH_FAIL(ICS_ERR_INVALID, "null argument");
  if (iface >= kNeighMaxIface) return NEIGH_FAIL(ICS_ERR_INVALID, "interface %u not below 65536", iface);
  std::lock_guard<std::mutex> lock(tbl->mu);
  return learn_locked(tbl, iface, ip, mac);
}

int ics_neigh_table_lookup(ics_neigh_table* tbl, uint32_t iface, uint32_t ip, uint8_t mac[6]) {
  if (!tbl || !mac) return NEIGH_FAIL(ICS_ERR_INVALID, "null argument");
  if (iface >= kNeighMaxIface) return NEIGH_FAIL(ICS_ERR_INVALID, "interface %u not below 65536", iface);
  std::lock_guard<std::mutex> lock(tbl->mu);
  if (int rc = compile(tbl)) return rc;
  const uint32_t* s = icsum::detail::neigh_walk(tbl->image.data() + 4 * tbl->ifaces.size(), tbl->nslots, iface, ip);
  if (!s) return 0;
  for (int k = 0; k < 4; ++k) mac[k] = uint8_t(s[2] >> (8 * k));
  mac[4] = uint8_t(s[3]);
  mac[5] = uint8_t(s[3] >> 8);
  return 1;
}

int ics_neigh_table_tick(ics_neigh_table* tbl, uint32_t iface, uint64_t ms) {
  if (!tbl) return NEIGH_FAIL(ICS_ERR_INVALID, "null neighbour table");
  if (iface != ICS_ALL_IFACES && iface >= kNeighMaxIface)
    return NEIGH_FAIL(ICS_ERR_INVALID, "interface %u not below 65536", iface);
  std::lock_guard<std::mutex> lock(tbl->mu);
  if (iface == ICS_ALL_IFACES) {
    for (Iface& it : tbl->ifaces) tick_one(tbl, it, ms);
  } else if (iface < tbl->ifaces.size()) {
    tick_one(tbl, tbl->ifaces[iface], ms);
  }
  return ICS_OK;
}

int ics_neigh_table_recv_frame(ics_neigh_table* tbl, uint32_t iface, const void* frame, size_t len, uint8_t* status,
                               uint32_t* events, uint32_t* sender_ip, void* reply42) {
  if (!tbl || !status || !events || !sender_ip || !reply42 || (!frame && len))
    return NEIGH_FAIL(ICS_ERR_INVALID, "null argument");
  if (iface >= kNeighMaxIface) return NEIGH_FAIL(ICS_ERR_INVALID, "interface %u not below 65536", iface);
  *status = 0;
  *events = 0;
  *sender_ip = 0;
  std::lock_guard<std::mutex> lock(tbl->mu);
  if (iface >= tbl->ifaces.size() || !tbl->ifaces[iface].set)
    return NEIGH_FAIL(ICS_ERR_INVALID, "interface %u has no addresses (ics_neigh_table_set_iface)", iface);
  const uint8_t* f = static_cast<const uint8_t*>(frame);
  if (len < 14) return ICS_OK;
  static const uint8_t kBroadcast[6] = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
  if (std::memcmp(f, kBroadcast, 6) != 0 && std::memcmp(f, tbl->ifaces[iface].mac, 6) != 0) return ICS_OK;
  uint8_t st = ICS_FR_FOR_US;
  const uint32_t type = be16(f + 12);
  const uint8_t* p = f + 14;
  const size_t plen = len - 14;
  if (type == 0x0800u) {
    st |= ICS_FR_IPV4;
    if (ipv4_parses(p, plen)) st |= ICS_FR_DGRAM;
  } else if (type == 0x0806u) {
    st |= ICS_FR_ARP;
    const uint32_t opcode = plen >= 8 ? be16(p + 6) : 0;
    if (plen >= 28 && be16(p) == 1 && be16(p + 2) == 0x0800u && p[4] == 6 && p[5] == 4 &&
        (opcode == 1 || opcode == 2)) {
      st |= ICS_FR_ARP_OK;
      const uint32_t sip = be32(p + 14), tip = be32(p + 24);
      uint8_t smac[6];
      std::memcpy(smac, p + 8, 6);
      if (int rc = learn_locked(tbl, iface, sip, smac)) return rc;
      const Iface& me = tbl->ifaces[iface];  // after learn_locked: it never moves an existing entry
      *sender_ip = sip;
      if (opcode == 1 && tip == me.ip) {
        arp_frame(static_cast<uint8_t*>(reply42), me, 2, sip, smac);
        *events = ICS_ARP_REPLY;
      } else if (opcode == 2) {
        *events = ICS_ARP_RELEASE;
      }
    }
  }
  *status = st;
  return ICS_OK;
}

int ics_neigh_table_resolve(ics_neigh_table* tbl, uint32_t iface, uint32_t next_hop, uint8_t hdr14[14],
                            uint32_t* events, void* request42) {
  if (!tbl || !hdr14 || !events || !request42) return NEIGH_FAIL(ICS_ERR_INVALID, "null argument");
  if (iface >= kNeighMaxIface) return NEIGH_FAIL(ICS_ERR_INVALID, "interface %u not below 65536", iface);
  *events = 0;
  std::lock_guard<std::mutex> lock(tbl->mu);
  if (iface >= tbl->ifaces.size() || !tbl->ifaces[iface].set) return 0;  // never resolved, nothing to send from
  Iface& me = tbl->ifaces[iface];
  auto hit = me.map.find(next_hop);
  if (hit != me.map.end()) {
    std::memcpy(hdr14, hit->second.mac, 6);
    std::memcpy(hdr14 + 6, me.mac, 6);
    hdr14[12] = 0x08, hdr14[13] = 0x00;
    return 1;
  }
  if (me.req.find(next_hop) == me.req.end()) {
    try {
      me.req.emplace(next_hop, 0u);
    } catch (const std::bad_alloc&) {
      return NEIGH_FAIL(ICS_ERR_NOMEM, "neighbour table allocation failed");
    }
    arp_frame(static_cast<uint8_t*>(request42), me, 1, next_hop, nullptr);
    *events = ICS_ARP_REQUEST;
  }
  return 0;
}

int ics_neigh_table_stats(ics_neigh_table* tbl, ics_neigh_stats_t* stats) {
  if (!tbl || !stats) return NEIGH_FAIL(ICS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(tbl->mu);
  if (int rc = compile(tbl)) return rc;
  ics_neigh_stats_t st{};
  for (const Iface& it : tbl->ifaces) {
    st.ifaces += it.set;
    st.pending_requests += it.req.size();
  }
  st.mappings = tbl->mappings;
  st.image_ifaces = tbl->ifaces.size();
  st.image_slots = tbl->nslots;
  st.generation = tbl->gen;
  *stats = st;
  return ICS_OK;
}

}  // extern "C"
