// gen_frame_golden.cpp — writes tests/golden/frame_cases.json from the real
// reference's NetworkInterface (src/network_interface/network_interface.cpp)
// and Router (src/router/router.cpp), driven through an OutputPort that
// records every transmitted frame.  Run once by hand where the reference tree
// is checked out; not part of build(), and nothing at test time needs it.  It
// includes the reference's headers and links its sources; it contains none of
// its text.
//
//   REF=<the reference tree>
//   g++ -std=gnu++20 -O1 -w $(for d in $REF/util/*/ $REF/src/*/; do echo -I$d; done)
//       tools/gen_frame_golden.cpp $REF/src/router/router.cpp
//       $REF/src/network_interface/network_interface.cpp $REF/util/address/address.cpp
//       $REF/util/ipv4_header/ipv4_header.cpp $REF/util/ethernet/ethernet_header.cpp
//       $REF/util/arp_message/arp_message.cpp -o gen_frame_golden
//   ./gen_frame_golden > tests/golden/frame_cases.json 2> /dev/null   # the constructors log to stderr
//
// Output: {"scenarios": [{"name", "ifaces": [[mac hex, ip], ...], "routes":
// [[prefix, len, iface, has_next_hop, next_hop], ...], "events": [...]}]}.  An
// event is {"op": "recv", "iface", "frame": hex, "tag"} (handed to recv_frame
// when it parses as an EthernetFrame, as the reference's app does), {"op":
// "tick", "iface" (-1: every interface), "ms"}, {"op": "route"} or {"op":
// "send", "iface", "dgram": hex, "next_hop"} (a direct send_datagram); each
// carries what followed: "tx": [[iface, frame hex], ...] in transmit order and
// "queued": the length of every interface's datagrams_received queue.
#include <array>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "router.h"

namespace {

using Bytes = std::string;
using Mac = std::array<uint8_t, 6>;

struct Port : NetworkInterface::OutputPort {
  std::vector<std::pair<int, Bytes>> sent;
  void transmit(const NetworkInterface& sender, const EthernetFrame& frame) override {
    Bytes all;
    for (const auto& piece : serialize(frame)) all += piece;
    sent.emplace_back(std::stoi(sender.name()), all);
  }
};

std::string hex(const Bytes& b) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (unsigned char c : b) {
    s += d[c >> 4];
    s += d[c & 15];
  }
  return s;
}

uint32_t ip(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a << 24 | b << 16 | c << 8 | d; }
void put16(Bytes& b, uint32_t v) {
  b += char(v >> 8);
  b += char(v);
}
void put32(Bytes& b, uint32_t v) {
  put16(b, v >> 16);
  put16(b, v & 0xffff);
}
Bytes mac_bytes(const Mac& m) { return Bytes(reinterpret_cast<const char*>(m.data()), 6); }

Bytes eth(const Mac& dst, const Mac& src, uint32_t type, const Bytes& payload) {
  Bytes f = mac_bytes(dst) + mac_bytes(src);
  put16(f, type);
  return f + payload;
}

struct Ip4 {
  uint32_t ver = 4, hlen = 5, ttl = 64, flags = 0x4000, src = 0, dst = 0;
  bool bad_ck = false;
  uint32_t payload = 8;  // bytes after the header (options included in hlen)
};

// a datagram whose checksum is the one IPv4Header::parse recomputes: over the
// 20 bytes with the checksum zero and the reserved flag bit dropped
Bytes ip4(const Ip4& h, int cut = -1) {
  Bytes b;
  b += char(h.ver << 4 | h.hlen);
  b += char(0);
  put16(b, 4 * h.hlen + h.payload);
  put16(b, 0x1234);
  put16(b, h.flags);
  b += char(h.ttl);
  b += char(17);
  put16(b, 0);
  put32(b, h.src);
  put32(b, h.dst);
  uint32_t s = 0;
  for (int k = 0; k < 20; k += 2) {
    uint32_t w = uint32_t(uint8_t(b[k])) << 8 | uint8_t(b[k + 1]);
    if (k == 6) w &= 0x7fff;
    s += w;
  }
  s = (s >> 16) + (s & 0xffff);
  s = (s >> 16) + (s & 0xffff);
  uint32_t ck = ~s & 0xffff;
  if (h.bad_ck) ck ^= 0x0100;
  b[10] = char(ck >> 8);
  b[11] = char(ck);
  for (uint32_t k = 20; k < 4 * h.hlen + h.payload; ++k) b += char(0xa0 + k % 80);
  if (cut >= 0) b.resize(cut);
  return b;
}

struct Arp {
  uint32_t hw = 1, proto = 0x0800, hs = 6, ps = 4, op = 1;
  Mac smac{}, tmac{};
  uint32_t sip = 0, tip = 0;
};

Bytes arp(const Arp& a, int size = 28) {
  Bytes b;
  put16(b, a.hw);
  put16(b, a.proto);
  b += char(a.hs);
  b += char(a.ps);
  put16(b, a.op);
  b += mac_bytes(a.smac);
  put32(b, a.sip);
  b += mac_bytes(a.tmac);
  put32(b, a.tip);
  b.resize(size, char(0));
  return b;
}

struct Scenario {
  std::string name;
  Router router;
  std::shared_ptr<Port> port = std::make_shared<Port>();
  std::vector<std::pair<Mac, uint32_t>> ifaces;
  std::string routes_json, events_json;

  explicit Scenario(std::string n) : name(std::move(n)) {}

  void iface(const Mac& m, uint32_t addr) {
    router.add_interface(std::make_shared<NetworkInterface>(std::to_string(ifaces.size()), port, m,
                                                            Address::from_ipv4_numeric(addr)));
    ifaces.emplace_back(m, addr);
  }
  void route(uint32_t prefix, uint32_t len, uint32_t ifc, bool has, uint32_t nh) {
    router.add_route(prefix, uint8_t(len), has ? std::optional<Address>(Address::from_ipv4_numeric(nh)) : std::nullopt,
                     ifc);
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s[%u, %u, %u, %d, %u]", routes_json.empty() ? "" : ", ", prefix, len, ifc,
                  int(has), nh);
    routes_json += buf;
  }
  void after(const std::string& head) {
    std::string e = "{" + head + ", \"tx\": [";
    for (size_t k = 0; k < port->sent.size(); ++k)
      e += std::string(k ? ", " : "") + "[" + std::to_string(port->sent[k].first) + ", \"" + hex(port->sent[k].second) +
           "\"]";
    port->sent.clear();
    e += "], \"queued\": [";
    for (size_t k = 0; k < ifaces.size(); ++k)
      e += std::string(k ? ", " : "") + std::to_string(router.interface(k)->datagrams_received().size());
    e += "]}";
    events_json += (events_json.empty() ? "\n  " : ",\n  ") + e;
  }
  void recv(size_t ifc, const Bytes& frame, const std::string& tag) {
    EthernetFrame f;
    if (parse(f, std::vector<std::string>{frame})) router.interface(ifc)->recv_frame(f);
    after("\"op\": \"recv\", \"iface\": " + std::to_string(ifc) + ", \"tag\": \"" + tag + "\", \"frame\": \"" +
          hex(frame) + "\"");
  }
  void tick(int ifc, size_t ms) {
    for (size_t k = 0; k < ifaces.size(); ++k)
      if (ifc < 0 || size_t(ifc) == k) router.interface(k)->tick(ms);
    after("\"op\": \"tick\", \"iface\": " + std::to_string(ifc) + ", \"ms\": " + std::to_string(ms));
  }
  void do_route() {
    router.route();
    after("\"op\": \"route\"");
  }
  void send(size_t ifc, const Bytes& dgram, uint32_t nh) {
    InternetDatagram d;
    if (!parse(d, std::vector<std::string>{dgram})) std::abort();
    router.interface(ifc)->send_datagram(d, Address::from_ipv4_numeric(nh));
    after("\"op\": \"send\", \"iface\": " + std::to_string(ifc) + ", \"next_hop\": " + std::to_string(nh) +
          ", \"dgram\": \"" + hex(dgram) + "\"");
  }
};

bool g_first = true;
void emit(Scenario& s) {
  std::printf("%s\n{\"name\": \"%s\", \"ifaces\": [", g_first ? "" : ",", s.name.c_str());
  g_first = false;
  for (size_t k = 0; k < s.ifaces.size(); ++k)
    std::printf("%s[\"%s\", %u]", k ? ", " : "", hex(mac_bytes(s.ifaces[k].first)).c_str(), s.ifaces[k].second);
  std::printf("],\n \"routes\": [%s],\n \"events\": [%s\n ]}", s.routes_json.c_str(), s.events_json.c_str());
}

const Mac kBcast = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff};
const Mac kM0 = {0x02, 0x00, 0x00, 0x00, 0x00, 0x10}, kM1 = {0x02, 0x00, 0x00, 0x00, 0x01, 0x11},
          kM2 = {0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0x12};
const Mac kOther = {0x02, 0x00, 0x00, 0x00, 0x00, 0x99}, kMulti = {0x01, 0x00, 0x5e, 0x00, 0x00, 0x01};
Mac host_mac(uint32_t k) { return {0x06, 0x11, uint8_t(k >> 24), uint8_t(k >> 16), uint8_t(k >> 8), uint8_t(k)}; }

Bytes plain_dgram(uint32_t dst, uint32_t payload = 8, uint32_t ttl = 64) {
  Ip4 h;
  h.src = ip(172, 16, 0, 9);
  h.dst = dst;
  h.payload = payload;
  h.ttl = ttl;
  return ip4(h);
}

}  // namespace

int main() {
  std::printf("{\"scenarios\": [");
  const uint32_t ip0 = ip(10, 0, 0, 1), ip1 = ip(10, 0, 1, 1), ip2 = ip(192, 168, 7, 1);

  {  // destination filter, frame types, frame lengths: one interface, nothing routed
    Scenario s("filter_types_lengths");
    s.iface(kM0, ip0);
    const Bytes d = plain_dgram(ip(10, 0, 0, 77), 8);
    s.recv(0, eth(kM0, kOther, 0x0800, d), "dst own");
    s.recv(0, eth(kBcast, kOther, 0x0800, d), "dst broadcast");
    s.recv(0, eth(kOther, kM0, 0x0800, d), "dst another unicast");
    s.recv(0, eth(kMulti, kOther, 0x0800, d), "dst multicast");
    Mac almost = kM0;
    almost[5] ^= 1;
    s.recv(0, eth(almost, kOther, 0x0800, d), "dst one bit off");
    Mac half_b = kBcast;
    half_b[4] = 0xfe;
    s.recv(0, eth(half_b, kOther, 0x0800, d), "dst almost broadcast");
    s.recv(0, eth(kM0, kOther, 0x0800, d), "type 0x0800");
    Arp a;
    a.smac = host_mac(1);
    a.sip = ip(10, 0, 0, 50);
    a.tip = ip0;
    s.recv(0, eth(kM0, host_mac(1), 0x0806, arp(a)), "type 0x0806");
    s.recv(0, eth(kM0, kOther, 0x86dd, d), "type 0x86DD");
    s.recv(0, eth(kM0, kOther, 0, d), "type 0");
    s.recv(0, eth(kM0, kOther, 0x0008, d), "type byte-swapped");
    const Bytes v4 = eth(kM0, kOther, 0x0800, d);  // 42 bytes
    a.sip = ip(10, 0, 0, 51);
    a.smac = host_mac(2);
    const Bytes va = eth(kBcast, host_mac(2), 0x0806, arp(a));  // 42 bytes
    for (int len : {0, 13, 14, 33, 34, 41, 42}) {
      s.recv(0, v4.substr(0, len), "length " + std::to_string(len) + " ipv4");
      s.recv(0, va.substr(0, len), "length " + std::to_string(len) + " arp");
    }
    s.send(0, plain_dgram(ip(10, 0, 0, 51)), ip(10, 0, 0, 51));  // learned from the 42-byte ARP alone
    emit(s);
  }

  {  // IPv4 parse and forward cases through a two-interface router, neighbours known
    Scenario s("ipv4_cases");
    s.iface(kM0, ip0);
    s.iface(kM1, ip1);
    s.route(ip(10, 0, 1, 0), 24, 1, false, 0);
    s.route(ip(10, 0, 0, 0), 24, 0, false, 0);
    const uint32_t dst = ip(10, 0, 1, 20);
    Arp a;
    a.op = 2;
    a.smac = host_mac(20);
    a.sip = dst;
    a.tip = ip1;
    a.tmac = kM1;
    s.recv(1, eth(kM1, host_mac(20), 0x0806, arp(a)), "learn the destination");
    auto one = [&](const std::string& tag, Ip4 h, int cut = -1) {
      h.src = ip(10, 0, 0, 5);
      h.dst = dst;
      s.recv(0, eth(kM0, kOther, 0x0800, ip4(h, cut)), tag);
    };
    Ip4 h;
    one("ipv4 valid", h);
    h.bad_ck = true;
    one("ipv4 bad checksum", h);
    h = Ip4{};
    h.ver = 6;
    one("ipv4 version 6", h);
    h = Ip4{};
    h.hlen = 4;
    h.payload = 12;
    one("ipv4 hlen 4", h);
    h = Ip4{};
    h.hlen = 15;
    h.payload = 0;
    one("ipv4 hlen 15 in a 20-byte payload", h, 20);
    h = Ip4{};
    one("ipv4 19-byte payload", h, 19);
    for (uint32_t ttl : {0u, 1u, 2u, 255u}) {
      h = Ip4{};
      h.ttl = ttl;
      one("ipv4 ttl " + std::to_string(ttl), h);
    }
    h = Ip4{};
    h.flags = 0xc000;
    one("ipv4 reserved flag set", h);
    h = Ip4{};
    h.flags = 0xa123;
    one("ipv4 reserved flag, more fragments, offset", h);
    h = Ip4{};
    h.hlen = 6;
    h.payload = 10;
    one("ipv4 options hlen 6", h);
    h = Ip4{};
    h.hlen = 15;
    h.payload = 24;
    one("ipv4 options hlen 15", h);
    h = Ip4{};
    h.payload = 0;
    one("ipv4 header only", h);
    h = Ip4{};
    h.payload = 64;
    one("ipv4 64-byte payload", h);
    s.do_route();
    emit(s);
  }

  {  // ARP: learning, replies, releases, supported(), sizes — one interface, direct sends
    Scenario s("arp_cases");
    s.iface(kM0, ip0);
    uint32_t next = 100;
    auto from = [&](uint32_t k) {
      Arp a;
      a.smac = host_mac(k);
      a.sip = ip(10, 0, 0, k);
      a.tip = ip(10, 0, 0, 200);
      return a;
    };
    auto probe = [&](uint32_t k) { s.send(0, plain_dgram(ip(10, 0, 0, k)), ip(10, 0, 0, k)); };
    Arp a = from(next);
    a.tip = ip0;
    s.recv(0, eth(kBcast, a.smac, 0x0806, arp(a)), "arp request for us");
    probe(next++);
    a = from(next);
    s.recv(0, eth(kBcast, a.smac, 0x0806, arp(a)), "arp request for another ip");
    probe(next++);
    // three datagrams wait for one address; the reply releases them
    const uint32_t w = next++;
    s.send(0, plain_dgram(ip(10, 9, 9, 1), 4), ip(10, 0, 0, w));
    s.send(0, plain_dgram(ip(10, 9, 9, 2), 12), ip(10, 0, 0, w));
    s.send(0, plain_dgram(ip(10, 9, 9, 3), 0), ip(10, 0, 0, w));
    a = from(w);
    a.op = 2;
    a.tip = ip0;
    a.tmac = kM0;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp reply releasing three waiting datagrams");
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "the same reply again releases nothing");
    probe(w);
    // a request from an awaited address learns it and releases nothing
    const uint32_t y = next++;
    probe(y);
    a = from(y);
    s.recv(0, eth(kBcast, a.smac, 0x0806, arp(a)), "arp request from an awaited ip");
    probe(y);
    a.op = 2;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "its reply releases the first");
    a = from(next);
    s.recv(0, eth(kOther, a.smac, 0x0806, arp(a)), "arp to another mac");
    probe(next++);
    a = from(next);
    a.hw = 2;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp hardware type 2");
    probe(next++);
    a = from(next);
    a.proto = 0x0801;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp protocol 0x0801");
    probe(next++);
    a = from(next);
    a.hs = 5;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp hardware size 5");
    probe(next++);
    a = from(next);
    a.ps = 5;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp protocol size 5");
    probe(next++);
    a = from(next);
    a.op = 0;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp opcode 0");
    probe(next++);
    a = from(next);
    a.op = 3;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp opcode 3");
    probe(next++);
    a = from(next);
    a.op = 0x0101;
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp opcode 0x0101");
    probe(next++);
    a = from(next);
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a, 27)), "arp 27 bytes");
    probe(next++);
    a = from(next);
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a, 46)), "arp 46 bytes (padded)");
    probe(next++);
    a = from(next);
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp learn");
    probe(next);
    a.smac = host_mac(0xabcdef);
    s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "arp re-learn overwriting the mac");
    probe(next++);
    emit(s);
  }

  {  // timers: hold-down, expiry, re-learn, per-interface caches
    Scenario s("timers");
    s.iface(kM0, ip0);
    s.iface(kM1, ip1);
    auto probe = [&](size_t ifc, uint32_t k) { s.send(ifc, plain_dgram(ip(10, 0, 0, k)), ip(10, 0, 0, k)); };
    auto learn = [&](size_t ifc, uint32_t k, const std::string& tag) {
      Arp a;
      a.smac = host_mac(k);
      a.sip = ip(10, 0, 0, k);
      a.tip = ip(10, 0, 0, 200);
      s.recv(ifc, eth(kBcast, a.smac, 0x0806, arp(a)), tag);
    };
    probe(0, 30);  // a miss: one request
    probe(0, 30);  // inside the hold-down: none
    s.tick(-1, 4999);
    probe(0, 30);
    s.tick(-1, 1);  // exactly 5000: still held
    probe(0, 30);
    s.tick(-1, 1);  // 5001: a request again
    probe(0, 30);
    learn(0, 31, "learn 31 on interface 0");
    s.tick(-1, 30000);  // exactly 30000: alive
    probe(0, 31);
    s.tick(-1, 1);  // 30001: gone
    probe(0, 31);
    learn(0, 32, "learn 32");
    s.tick(-1, 20000);
    learn(0, 32, "re-learn 32 resets its timer");
    s.tick(-1, 20000);
    probe(0, 32);  // 40000 since the first learn, 20000 since the second: alive
    s.tick(-1, 10001);
    probe(0, 32);  // gone
    learn(0, 33, "learn 33 on interface 0 only");
    probe(1, 33);  // invisible on interface 1: a request there
    probe(0, 33);
    learn(1, 34, "learn 34 on interface 1");
    s.tick(0, 30001);  // only interface 0 ages
    probe(1, 34);      // alive on 1
    probe(0, 33);      // gone on 0
    // the reply does not erase the pending request: a miss after the mapping expired, inside 5 s, stays quiet
    probe(0, 35);
    {
      Arp a;
      a.op = 2;
      a.smac = host_mac(35);
      a.sip = ip(10, 0, 0, 35);
      a.tip = ip0;
      a.tmac = kM0;
      s.recv(0, eth(kM0, a.smac, 0x0806, arp(a)), "reply for 35 releases it");
    }
    probe(0, 35);
    emit(s);
  }

  {  // the whole hop: three interfaces, direct and next-hop routes, two bursts
    Scenario s("whole_hop");
    s.iface(kM0, ip0);
    s.iface(kM1, ip1);
    s.iface(kM2, ip2);
    s.route(ip(10, 0, 0, 0), 24, 0, false, 0);
    s.route(ip(10, 0, 1, 0), 24, 1, false, 0);
    s.route(ip(192, 168, 7, 0), 24, 2, false, 0);
    s.route(ip(172, 16, 0, 0), 12, 2, true, ip(192, 168, 7, 254));
    s.route(ip(8, 8, 0, 0), 16, 1, true, ip(10, 0, 1, 254));
    auto reply = [&](size_t ifc, const Mac& me, uint32_t my_ip, uint32_t k, uint32_t addr, const std::string& tag) {
      Arp a;
      a.op = 2;
      a.smac = host_mac(k);
      a.sip = addr;
      a.tip = my_ip;
      a.tmac = me;
      s.recv(ifc, eth(me, a.smac, 0x0806, arp(a)), tag);
    };
    auto dg = [&](size_t ifc, const Mac& me, uint32_t dst, uint32_t ttl, uint32_t payload, const std::string& tag) {
      Ip4 h;
      h.src = ip(10, 0, 0, 5);
      h.dst = dst;
      h.ttl = ttl;
      h.payload = payload;
      s.recv(ifc, eth(me, kOther, 0x0800, ip4(h)), tag);
    };
    // burst 1: neighbours arrive in the same burst as the traffic (recv_frame runs before route())
    reply(1, kM1, ip1, 0x120, ip(10, 0, 1, 20), "neighbour 10.0.1.20 on 1");
    reply(2, kM2, ip2, 0x2fe, ip(192, 168, 7, 254), "gateway 192.168.7.254 on 2");
    reply(0, kM0, ip0, 0x007, ip(10, 0, 0, 7), "neighbour 10.0.0.7 on 0");
    dg(0, kM0, ip(10, 0, 1, 20), 64, 8, "hop resolved direct");
    dg(0, kM0, ip(172, 20, 1, 1), 9, 16, "hop resolved via gateway");
    dg(0, kM0, ip(10, 0, 1, 20), 1, 8, "hop ttl expired");
    dg(0, kM0, ip(11, 1, 1, 1), 64, 8, "hop unrouted");
    dg(0, kM0, ip(10, 0, 1, 21), 64, 8, "hop routed, unresolved direct");
    dg(0, kM0, ip(8, 8, 8, 8), 64, 8, "hop routed, unresolved gateway");
    dg(0, kBcast, ip(10, 0, 1, 20), 2, 1480, "hop mtu frame, broadcast dst");
    dg(1, kM1, ip(10, 0, 0, 7), 64, 5, "hop from interface 1 to 0");
    dg(1, kM1, ip(8, 8, 4, 4), 64, 3, "hop second waiter for the gateway on 1");
    dg(1, kM1, ip(10, 0, 1, 21), 64, 7, "hop second waiter for 10.0.1.21");
    dg(2, kM2, ip(10, 0, 1, 20), 3, 1480, "hop mtu frame from interface 2");
    dg(2, kM2, ip(192, 168, 7, 254), 64, 2, "hop back out of its ingress interface");
    dg(2, kM0, ip(10, 0, 1, 20), 64, 8, "hop wrong interface's address");
    dg(2, kM2, ip(10, 0, 0, 7), 0, 8, "hop ttl 0");
    s.do_route();
    // burst 2: the missing neighbours answer, more traffic follows
    reply(1, kM1, ip1, 0x1fe, ip(10, 0, 1, 254), "gateway 10.0.1.254 answers: two released");
    reply(1, kM1, ip1, 0x121, ip(10, 0, 1, 21), "10.0.1.21 answers: two released");
    dg(0, kM0, ip(8, 8, 8, 8), 64, 8, "hop now resolved via gateway");
    dg(2, kM2, ip(10, 0, 1, 21), 2, 30, "hop now resolved direct");
    dg(0, kM0, ip(10, 0, 0, 9), 64, 8, "hop unresolved on its own ingress interface");
    s.do_route();
    s.tick(-1, 30001);
    dg(0, kM0, ip(10, 0, 1, 20), 64, 8, "hop after every mapping expired");
    s.do_route();
    emit(s);
  }

  std::printf("\n]}\n");
  return 0;
}
