// gen_unwrap_golden.cpp — writes tests/golden/unwrap_cases.json from the real
// reference's IPv4Datagram / TCPSegment parsers and TCPOverIPv4Adapter
// (util/ipv4_header, util/tcp_segment, util/tcp_over_ip).  Run once by hand
// where the reference tree is checked out; not part of build(), and nothing at
// test time needs it.  It includes the reference's headers and links its
// sources; it contains none of its text.  The wire datagrams are built here,
// byte by byte; everything recorded about them is what the reference said.
//
//   REF=<the reference tree>
//   g++ -std=gnu++20 -O1 -w $(for d in $REF/util/*/ $REF/src/*/; do echo -I$d; done)
//       tools/gen_unwrap_golden.cpp $REF/util/tcp_over_ip/tcp_over_ip.cpp
//       $REF/util/tcp_segment/tcp_segment.cpp $REF/util/ipv4_header/ipv4_header.cpp
//       $REF/util/address/address.cpp -o gen_unwrap_golden
//   ./gen_unwrap_golden > tests/golden/unwrap_cases.json
//
// Output: {"cases": [...], "scenarios": [...]}.
// A case is {"tag", "wire": hex, "ip_parse_ok": parse(IPv4Datagram, wire),
// "proto": header.proto after that parse, "tcp_parse_ok": parse(TCPSegment,
// dgram.payload, header.pseudo_checksum()) (false when the datagram did not
// parse)} and, where both parse, "src", "dst", "ttl", "id", "src_port",
// "dst_port", "seqno", "has_ack", "ackno" (0 without one), "syn", "fin", "rst",
// "window", "payload": hex.
// A scenario is {"name", "listening", "source": [ip, port], "destination":
// [ip, port], "dgrams": [{"tag", "wire", "unwrap_ok"}], "end_listening",
// "end_destination": [ip, port]}: one adapter fed the datagrams in order,
// unwrap_ok = the datagram parsed and unwrap_tcp_in_ip returned a message.
#include <cstdint>
#include <cstdio>
#include <optional>
#include <string>
#include <vector>

#include "ipv4_datagram.h"
#include "tcp_over_ip.h"
#include "tcp_segment.h"

namespace {

using Bytes = std::string;

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
void set16(Bytes& b, size_t at, uint32_t v) {
  b[at] = char(v >> 8);
  b[at + 1] = char(v);
}
uint32_t fold(uint32_t s) {
  while (s > 0xffff) s = (s >> 16) + (s & 0xffff);
  return ~s & 0xffff;
}
uint8_t at(const Bytes& b, size_t k) { return static_cast<uint8_t>(b[k]); }

// deterministic filler
uint32_t g_state = 0x756e7772;
uint32_t next() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state >> 8;
}
Bytes filler(size_t n) {
  Bytes b(n, '\0');
  for (auto& c : b) c = char(next());
  return b;
}

struct Dgram {
  uint32_t ver = 4, hlen = 5, tos = 0, id = 0x1234, frag = 0x4000, ttl = 64, proto = 6;
  uint32_t src = ip(10, 9, 8, 7), dst = ip(10, 1, 2, 3);
  uint32_t sport = 80, dport = 4321, seqno = 0x01020304, ackno = 0xa1b2c3d4, doff = 5, flags = 0x10, window = 0xfff0,
           urgent = 0;
  int tcp_opt_bytes = -1;  // bytes of TCP options present (-1: what doff claims)
  Bytes payload;
  Bytes trailing;          // bytes behind what the header's len counts
  bool bad_ip_ck = false, bad_tcp_ck = false;
  int cut = -1;            // keep only this many bytes of the finished datagram
};

// The datagram's bytes with both checksums as the reference's parsers
// recompute them: the header's over its 20 fixed bytes with the checksum zero
// and the reserved flag bit dropped, TCP's over the pseudo header and every
// byte behind the IPv4 header (its own field zero), trailing bytes included.
Bytes build(const Dgram& g) {
  Bytes b;
  b += char(g.ver << 4 | g.hlen);
  b += char(g.tos);
  put16(b, 0);
  put16(b, g.id);
  put16(b, g.frag);
  b += char(g.ttl);
  b += char(g.proto);
  put16(b, 0);
  put32(b, g.src);
  put32(b, g.dst);
  if (g.hlen > 5) b += filler(4 * (g.hlen - 5));
  const size_t t = b.size();
  put16(b, g.sport);
  put16(b, g.dport);
  put32(b, g.seqno);
  put32(b, g.ackno);
  b += char(g.doff << 4);
  b += char(g.flags);
  put16(b, g.window);
  put16(b, 0);
  put16(b, g.urgent);
  const int opt = g.tcp_opt_bytes >= 0 ? g.tcp_opt_bytes : (g.doff > 5 ? 4 * (int(g.doff) - 5) : 0);
  b += filler(opt);
  b += g.payload;
  const uint32_t len = uint32_t(b.size()) & 0xffff;
  b += g.trailing;
  if (g.cut >= 0 && size_t(g.cut) < b.size()) b.resize(g.cut);
  const uint32_t len_field = g.cut >= 0 ? uint32_t(b.size()) & 0xffff : len;
  if (b.size() >= 4) set16(b, 2, len_field);
  if (b.size() >= t + 18) {
    uint32_t s = (g.src >> 16) + (g.src & 0xffff) + (g.dst >> 16) + (g.dst & 0xffff) + g.proto +
                 ((len_field - 4 * g.hlen) & 0xffff);
    for (size_t k = t; k < b.size(); ++k) s += (k - t) & 1 ? at(b, k) : at(b, k) << 8;
    set16(b, t + 16, fold(s) ^ (g.bad_tcp_ck ? 0x0100 : 0));
  }
  if (b.size() >= 20) {
    uint32_t s = 0;
    for (size_t k = 0; k < 20; k += 2) {
      uint32_t w = at(b, k) << 8 | at(b, k + 1);
      if (k == 6) w &= 0x7fff;
      s += w;
    }
    set16(b, 10, fold(s) ^ (g.bad_ip_ck ? 0x0001 : 0));
  }
  return b;
}

class Wrap32Raw : public Wrap32 {
 public:
  explicit Wrap32Raw(Wrap32 w) : Wrap32(w) {}
  uint32_t raw() const { return raw_value_; }
};

bool first = true;
void sep() {
  std::printf(first ? "\n" : ",\n");
  first = false;
}

void emit_case(const char* tag, const Bytes& wire) {
  InternetDatagram d;
  const bool ip_ok = parse(d, std::vector<std::string>{wire});
  TCPSegment seg;
  const bool tcp_ok = ip_ok && parse(seg, d.payload, d.header.pseudo_checksum());
  sep();
  std::printf("  {\"tag\": \"%s\", \"wire\": \"%s\", \"ip_parse_ok\": %s, \"proto\": %u, \"tcp_parse_ok\": %s", tag,
              hex(wire).c_str(), ip_ok ? "true" : "false", unsigned(d.header.proto), tcp_ok ? "true" : "false");
  if (ip_ok && tcp_ok) {
    const TCPMessage& m = seg.message;
    const bool has_ack = m.receiver.ackno.has_value();
    std::printf(",\n   \"src\": %u, \"dst\": %u, \"ttl\": %u, \"id\": %u, \"src_port\": %u, \"dst_port\": %u, "
                "\"seqno\": %u, \"has_ack\": %s, \"ackno\": %u, \"syn\": %s, \"fin\": %s, \"rst\": %s, \"window\": %u, "
                "\"payload\": \"%s\"",
                d.header.src, d.header.dst, unsigned(d.header.ttl), unsigned(d.header.id), unsigned(seg.udinfo.src_port),
                unsigned(seg.udinfo.dst_port), Wrap32Raw(m.sender.seqno).raw(), has_ack ? "true" : "false",
                has_ack ? Wrap32Raw(*m.receiver.ackno).raw() : 0u, m.sender.SYN ? "true" : "false",
                m.sender.FIN ? "true" : "false", (m.sender.RST || m.receiver.RST) ? "true" : "false",
                unsigned(m.receiver.window_size), hex(m.sender.payload).c_str());
  }
  std::printf("}");
}

struct Step {
  const char* tag;
  Bytes wire;
};

void emit_scenario(const char* name, bool listening, const char* src_ip, uint16_t src_port, const char* dst_ip,
                   uint16_t dst_port, const std::vector<Step>& steps) {
  TCPOverIPv4Adapter a;
  a.config_mut().source = Address{src_ip, src_port};
  if (dst_ip) a.config_mut().destination = Address{dst_ip, dst_port};
  a.set_listening(listening);
  sep();
  std::printf("  {\"name\": \"%s\", \"listening\": %s, \"source\": [%u, %u], \"destination\": [%u, %u], \"dgrams\": [",
              name, listening ? "true" : "false", a.config().source.ipv4_numeric(), unsigned(a.config().source.port()),
              a.config().destination.ipv4_numeric(), unsigned(a.config().destination.port()));
  bool f = true;
  for (const Step& s : steps) {
    InternetDatagram d;
    const bool ok = parse(d, std::vector<std::string>{s.wire}) && a.unwrap_tcp_in_ip(d).has_value();
    std::printf("%s\n    {\"tag\": \"%s\", \"wire\": \"%s\", \"unwrap_ok\": %s}", f ? "" : ",", s.tag, hex(s.wire).c_str(),
                ok ? "true" : "false");
    f = false;
  }
  std::printf("],\n   \"end_listening\": %s, \"end_destination\": [%u, %u]}", a.listening() ? "true" : "false",
              a.config().destination.ipv4_numeric(), unsigned(a.config().destination.port()));
}

Dgram with_payload(size_t n) {
  Dgram g;
  g.payload = filler(n);
  return g;
}

}  // namespace

int main() {
  std::printf("{\"cases\": [");
  // ---- lengths
  emit_case("len_0", Bytes{});
  {
    Dgram g;
    g.cut = 19;
    emit_case("len_19", build(g));
    g.cut = 20;
    emit_case("len_20", build(g));
    g.cut = 39;  // 19 bytes of TCP whose checksum verifies: the header parse is what fails
    emit_case("len_39", build(g));
  }
  emit_case("len_40", build(Dgram{}));
  emit_case("len_41_odd_payload", build(with_payload(1)));
  emit_case("len_42_even_payload", build(with_payload(2)));
  emit_case("len_1500", build(with_payload(1460)));
  emit_case("payload_odd_333", build(with_payload(333)));
  emit_case("payload_even_1000", build(with_payload(1000)));
  // ---- IPv4 header shapes
  {
    Dgram g = with_payload(24);
    g.hlen = 6;
    emit_case("hlen_6", build(g));
    g.hlen = 15;
    emit_case("hlen_15", build(g));
    Dgram h;
    h.hlen = 15;
    h.cut = 60;  // the options fill the datagram: the TCP part is empty
    emit_case("hlen_15_len_60", build(h));
    Dgram k;
    k.hlen = 6;
    k.cut = 43;  // 19 bytes of TCP behind 24 of header
    emit_case("hlen_6_len_43", build(k));
    Dgram k44;
    k44.hlen = 6;  // exactly a TCP header behind the options
    emit_case("hlen_6_len_44", build(k44));
    Dgram v6 = with_payload(8);
    v6.ver = 6;
    emit_case("version_6", build(v6));
    Dgram h4 = with_payload(8);
    h4.hlen = 4;
    emit_case("hlen_4", build(h4));
    Dgram bi = with_payload(8);
    bi.bad_ip_ck = true;
    emit_case("bad_ip_checksum", build(bi));
    Dgram bt = with_payload(8);
    bt.bad_tcp_ck = true;
    emit_case("bad_tcp_checksum", build(bt));
    Dgram udp = with_payload(8);
    udp.proto = 17;
    emit_case("proto_17_verifies", build(udp));
    Dgram urg = with_payload(5);
    urg.urgent = 0x0102;
    emit_case("urgent_nonzero", build(urg));
    Dgram tos = with_payload(5);
    tos.tos = 0xb8;
    emit_case("tos_nonzero", build(tos));
    Dgram mf = with_payload(5);
    mf.frag = 0x2000;
    emit_case("fragment_mf", build(mf));
    Dgram rsv = with_payload(5);
    rsv.frag = 0xc000;  // the reserved bit: dropped from the checksum the parser recomputes
    emit_case("fragment_reserved_bit", build(rsv));
    Dgram tr = with_payload(10);
    tr.trailing = filler(7);
    emit_case("trailing_beyond_len", build(tr));
    Dgram ttl = with_payload(3);
    ttl.ttl = 1;
    ttl.id = 0xfffe;
    ttl.src = 0xffffffff;
    ttl.dst = 0;
    emit_case("edge_addresses_ttl_id", build(ttl));
  }
  // ---- TCP header shapes
  {
    Dgram d4 = with_payload(8);
    d4.doff = 4;
    emit_case("doff_4", build(d4));
    Dgram d6 = with_payload(9);
    d6.doff = 6;
    emit_case("doff_6", build(d6));
    Dgram d15 = with_payload(9);
    d15.doff = 15;
    emit_case("doff_15", build(d15));
    Dgram d15e;
    d15e.doff = 15;  // the options end exactly at the datagram's end
    emit_case("doff_15_exact_end", build(d15e));
    Dgram d15p;
    d15p.doff = 15;
    d15p.tcp_opt_bytes = 12;  // claims 40 bytes of options, holds 12: empty payload, still parses
    emit_case("doff_15_past_end", build(d15p));
    Dgram d6p;
    d6p.doff = 6;
    d6p.tcp_opt_bytes = 0;
    emit_case("doff_6_past_end", build(d6p));
    Dgram d6o = with_payload(4);
    d6o.hlen = 6;
    d6o.doff = 6;
    emit_case("hlen_6_doff_6", build(d6o));
    Dgram d15o = with_payload(4);
    d15o.hlen = 15;
    d15o.doff = 15;
    emit_case("hlen_15_doff_15", build(d15o));
    Dgram ff = with_payload(6);
    ff.flags = 0xff;
    emit_case("flags_ff", build(ff));
    Dgram f0 = with_payload(6);
    f0.flags = 0x00;  // no ACK bit, a nonzero ackno on the wire
    emit_case("flags_00_ackno_on_wire", build(f0));
    Dgram syn;
    syn.flags = 0x02;
    syn.ackno = 0;
    emit_case("syn", build(syn));
    Dgram fin = with_payload(1);
    fin.flags = 0x11;
    emit_case("fin_ack", build(fin));
    Dgram rst;
    rst.flags = 0x04;
    emit_case("rst", build(rst));
    Dgram edge = with_payload(2);
    edge.sport = 0xffff;
    edge.dport = 0;
    edge.seqno = 0xffffffff;
    edge.ackno = 0x80000000;
    edge.window = 0;
    emit_case("edge_ports_seqno_window", build(edge));
  }
  std::printf("\n],\n\"scenarios\": [");
  first = true;
  // ---- adapter scenarios
  auto from = [](uint32_t src, uint32_t sport, uint32_t dst, uint32_t dport, uint32_t flags, size_t payload) {
    Dgram g = with_payload(payload);
    g.src = src;
    g.sport = sport;
    g.dst = dst;
    g.dport = dport;
    g.flags = flags;
    return g;
  };
  const uint32_t me = ip(10, 1, 2, 3), peer = ip(10, 9, 8, 7), other = ip(10, 9, 8, 9);
  emit_scenario("listening_connects_on_third", true, "0", 4321, nullptr, 0,
                {{"data_before_syn", build(from(peer, 80, me, 4321, 0x10, 100))},
                 {"syn_rst", build(from(peer, 80, me, 4321, 0x06, 0))},
                 {"syn_connects", build(from(peer, 80, me, 4321, 0x02, 0))},
                 {"peer_data", build(from(peer, 80, me, 4321, 0x10, 333))},
                 {"stranger_data", build(from(other, 80, me, 4321, 0x10, 10))},
                 {"peer_data_again", build(from(peer, 80, me, 4321, 0x18, 1000))}});
  {
    Dgram noproto = from(peer, 80, me, 4321, 0x10, 4);
    noproto.proto = 17;
    Dgram bad = from(peer, 80, me, 4321, 0x10, 40);
    bad.bad_tcp_ck = true;
    Dgram opt = from(peer, 80, me, 4321, 0x18, 50);
    opt.hlen = 7;
    opt.doff = 8;
    emit_scenario("listening", true, "0", 4321, nullptr, 0,
                  {{"data_before_syn", build(from(peer, 80, me, 4321, 0x10, 100))},
                   {"syn_rst", build(from(peer, 80, me, 4321, 0x06, 0))},
                   {"syn_wrong_dport", build(from(peer, 80, me, 4322, 0x02, 0))},
                   {"syn_bad_checksum", build([&] { Dgram s = from(peer, 80, me, 4321, 0x02, 0); s.bad_tcp_ck = true; return s; }())},
                   {"syn_connects", build(from(peer, 80, me, 4321, 0x02, 0))},
                   {"peer_data", build(from(peer, 80, me, 4321, 0x10, 333))},
                   {"stranger_data", build(from(other, 80, me, 4321, 0x10, 10))},
                   {"stranger_syn", build(from(other, 80, me, 4321, 0x02, 0))},
                   {"peer_other_port", build(from(peer, 81, me, 4321, 0x10, 7))},
                   {"peer_to_other_dst", build(from(peer, 80, ip(10, 1, 2, 4), 4321, 0x10, 7))},
                   {"peer_proto_17", build(noproto)},
                   {"peer_bad_checksum", build(bad)},
                   {"peer_with_options", build(opt)},
                   {"peer_second_syn", build(from(peer, 80, me, 4321, 0x12, 0))},
                   {"peer_fin", build(from(peer, 80, me, 4321, 0x11, 1))}});
  }
  {
    Dgram noproto = from(peer, 80, me, 4321, 0x10, 64);
    noproto.proto = 17;
    Dgram short39 = from(peer, 80, me, 4321, 0x10, 0);
    short39.cut = 39;
    Dgram d4 = from(peer, 80, me, 4321, 0x10, 8);
    d4.doff = 4;
    Dgram badip = from(peer, 80, me, 4321, 0x10, 8);
    badip.bad_ip_ck = true;
    emit_scenario("connected", false, "10.1.2.3", 4321, "10.9.8.7", 80,
                  {{"passes", build(from(peer, 80, me, 4321, 0x10, 64))},
                   {"wrong_src", build(from(other, 80, me, 4321, 0x10, 64))},
                   {"wrong_dst", build(from(peer, 80, ip(10, 1, 2, 4), 4321, 0x10, 64))},
                   {"wrong_sport", build(from(peer, 81, me, 4321, 0x10, 64))},
                   {"wrong_dport", build(from(peer, 80, me, 4322, 0x10, 64))},
                   {"wrong_proto", build(noproto)},
                   {"truncated_39", build(short39)},
                   {"doff_4", build(d4)},
                   {"bad_ip_checksum", build(badip)},
                   {"syn_from_peer", build(from(peer, 80, me, 4321, 0x02, 0))},
                   {"rst_from_peer", build(from(peer, 80, me, 4321, 0x14, 0))},
                   {"passes_again", build(from(peer, 80, me, 4321, 0x18, 1000))}});
  }
  std::printf("\n]}\n");
  return 0;
}
