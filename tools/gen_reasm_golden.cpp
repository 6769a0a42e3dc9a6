// gen_reasm_golden.cpp — writes tests/golden/reasm_cases.json from the real
// reference's TCPReceiver, Reassembler, ByteStream and Wrap32
// (src/tcp_receiver, src/reassembler, src/byte_stream, src/wrapping_integers).
// Run once by hand where the reference tree is checked out; not part of
// build(), and nothing at test time needs it.  It includes the reference's
// headers and links its sources; it contains none of its text.  The scenarios
// are built here; everything recorded about them is what the reference said.
//
//   REF=<the reference tree>
//   g++ -std=gnu++20 -O1 -w $(for d in $REF/util/*/ $REF/src/*/; do echo -I$d; done)
//       tools/gen_reasm_golden.cpp $REF/src/tcp_receiver/tcp_receiver.cpp
//       $REF/src/reassembler/reassembler.cpp $REF/src/byte_stream/byte_stream.cpp
//       $REF/src/wrapping_integers/wrapping_integers.cpp -o gen_reasm_golden
//   ./gen_reasm_golden 2>/dev/null > tests/golden/reasm_cases.json
//
// Output: {"scenarios": [{"tag", "capacity", "ops": [...]}]}.  An op is
//   {"op": "recv", "seqno", "syn", "fin", "rst", "payload": hex}
//   {"op": "pop", "n"}          read(reader, n): "popped": hex of what it returned
//   {"op": "set_error"}         reader().set_error()
// each with the reference's answers after it: "pushed" (writer().bytes_pushed()),
// "pending" (reassembler().bytes_pending()), "avail" (available_capacity()),
// "closed", "error", and send()'s "ackno" (raw, null when absent), "window",
// "rst".
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "tcp_receiver.h"

namespace {

struct Op {
  int kind;  // 0 recv, 1 pop, 2 set_error
  uint32_t seqno = 0;
  bool syn = false, fin = false, rst = false;
  std::string payload;
  uint64_t n = 0;
};
struct Scenario {
  std::string tag;
  uint64_t capacity;
  std::vector<Op> ops;
};

std::vector<Scenario> g_all;
Scenario* g_cur = nullptr;
uint32_t g_isn = 0;

// the stream's byte at index i as sender `salt` would send it: salt 0 is the
// stream every agreeing segment carries, another salt a conflicting copy
char byte_at(uint64_t i, unsigned salt) { return char((i * 131u + (i >> 8) * 17u + 7u + salt * 89u) & 0xffu); }
std::string pay(uint64_t idx, uint64_t len, unsigned salt = 0) {
  std::string s(len, '\0');
  for (uint64_t k = 0; k < len; ++k) s[k] = byte_at(idx + k, salt);
  return s;
}

void begin(const std::string& tag, uint64_t cap, uint32_t isn = 1000) {
  g_all.push_back(Scenario{tag, cap, {}});
  g_cur = &g_all.back();
  g_isn = isn;
}
void raw(uint32_t seqno, const std::string& payload, bool syn = false, bool fin = false, bool rst = false) {
  Op o{0};
  o.seqno = seqno, o.syn = syn, o.fin = fin, o.rst = rst, o.payload = payload;
  g_cur->ops.push_back(o);
}
void syn(const std::string& payload = "", bool fin = false) { raw(g_isn, payload, true, fin); }
// a data segment at stream index idx (seqno isn + 1 + idx)
void seg(uint64_t idx, uint64_t len, unsigned salt = 0, bool fin = false) {
  raw(g_isn + 1u + uint32_t(idx), pay(idx, len, salt), false, fin);
}
void pop(uint64_t n) {
  Op o{1};
  o.n = n;
  g_cur->ops.push_back(o);
}
void set_error() { g_cur->ops.push_back(Op{2}); }

struct Range {
  uint64_t idx, len;
  unsigned salt;
};
// pending intervals behind a hole at [0, 4), then the hole filled and all popped:
// the popped bytes say which source won every overlap
void merge_case(const std::string& tag, const std::vector<Range>& rs) {
  for (int conflict = 0; conflict < 2; ++conflict) {
    begin("merge_" + tag + (conflict ? "_conflict" : "_agree"), 64);
    syn();
    unsigned k = 0;
    for (const Range& r : rs) seg(r.idx, r.len, conflict ? ++k : 0);
    seg(0, 4);
    pop(64);
  }
}

void build() {
  begin("in_order", 64);
  syn(); seg(0, 5); seg(5, 7); seg(12, 1); pop(13);
  begin("reversed", 64);
  syn(); seg(12, 4); seg(8, 4); seg(4, 4); seg(0, 4); pop(16);
  begin("holes_interleaved", 64);
  syn(); seg(2, 2); seg(6, 2); seg(10, 2); seg(4, 2); seg(0, 2); pop(5); seg(8, 2); pop(64);

  merge_case("touch_prev", {{4, 4, 0}, {8, 4, 0}});
  merge_case("inside_prev", {{4, 10, 0}, {6, 3, 0}});
  merge_case("inside_prev_same_end", {{4, 10, 0}, {6, 8, 0}});
  merge_case("overlap_prev", {{4, 6, 0}, {7, 6, 0}});
  merge_case("same_beg_longer", {{4, 4, 0}, {4, 9, 0}});
  merge_case("same_beg_shorter", {{4, 9, 0}, {4, 4, 0}});
  merge_case("duplicate_pending", {{4, 6, 0}, {4, 6, 0}});
  merge_case("next_keeps", {{8, 6, 0}, {4, 7, 0}});
  merge_case("next_covered", {{8, 3, 0}, {4, 10, 0}});
  merge_case("next_touch", {{8, 4, 0}, {4, 4, 0}});
  merge_case("next_same_end", {{8, 4, 0}, {4, 8, 0}});
  merge_case("bridge", {{4, 4, 0}, {12, 4, 0}, {20, 6, 0}, {6, 16, 0}});
  merge_case("bridge_all_covered", {{6, 2, 0}, {10, 2, 0}, {14, 2, 0}, {4, 20, 0}});
  merge_case("prev_and_next", {{4, 6, 0}, {14, 6, 0}, {8, 8, 0}});
  merge_case("first_position", {{10, 4, 0}, {4, 3, 0}});
  merge_case("first_position_overlap", {{10, 4, 0}, {4, 8, 0}});

  begin("duplicate_pushed", 64);
  syn(); seg(0, 6); seg(0, 6, 1); seg(2, 3, 2); pop(64);
  begin("straddle_unassembled", 64);
  syn(); seg(0, 6); seg(3, 8, 1); seg(20, 4); seg(8, 14, 2); pop(64);

  begin("edge_straddle", 16);
  syn(); seg(0, 4); seg(10, 10); seg(4, 6); pop(64);
  begin("edge_at", 16);
  syn(); seg(16, 4); seg(15, 4); seg(0, 15); pop(64);
  begin("edge_past", 16);
  syn(); seg(17, 4); seg(40, 1); seg(0, 3); pop(3);
  begin("edge_after_pop", 16);
  syn(); seg(0, 10); seg(14, 6); pop(4); seg(14, 6, 1); seg(18, 4); seg(20, 1); seg(10, 4); pop(64); seg(20, 20); pop(64);

  begin("cap1", 1);
  syn(); seg(0, 3); seg(1, 1); pop(1); seg(1, 2); seg(2, 1, 1); pop(1); seg(2, 1); pop(1);
  begin("cap2", 2);
  syn(); seg(1, 3); seg(0, 1); pop(1); seg(2, 2); pop(2); seg(3, 1, 0, true); pop(2);
  begin("cap7", 7);
  syn(); seg(3, 10); seg(0, 3); pop(5); seg(7, 9, 1); pop(7); seg(12, 3); pop(7);
  begin("cap65535", 65535);
  syn(); seg(0, 1000); seg(65000, 1000); pop(600); seg(65535, 700); seg(66135, 10); pop(400);
  begin("cap70000_window", 70000);
  syn(); seg(0, 3000); seg(69990, 20); pop(3000);

  begin("wrap_many", 10);
  syn();
  for (uint64_t at = 0; at < 73; at += 7) {
    seg(at + 3, 4);
    seg(at, 3);
    seg(at + 5, 5, 1);  // clipped at the edge, and its start already held
    pop(7);
  }
  pop(64);

  begin("fin_in_order", 64);
  syn(); seg(0, 5); seg(5, 3, 0, true); pop(64);
  begin("fin_early", 64);
  syn(); seg(5, 3, 0, true); seg(8, 2); seg(0, 5); pop(64);
  begin("fin_empty", 64);
  syn(); seg(0, 5); seg(5, 0, 0, true); pop(64);
  begin("fin_empty_early", 64);
  syn(); seg(5, 0, 0, true); seg(0, 4); seg(4, 1); pop(64);
  begin("fin_duplicated", 64);
  syn(); seg(3, 3, 0, true); seg(3, 3, 0, true); seg(0, 3); seg(3, 3, 0, true); pop(64);
  begin("fin_moved_earlier", 64);
  syn(); seg(6, 2, 0, true); seg(2, 2, 0, true); seg(0, 2); seg(4, 2); pop(64);
  begin("fin_behind_window", 8);
  syn(); seg(8, 2, 0, true); seg(12, 0, 0, true); seg(0, 8); pop(8); seg(8, 2, 0, true); pop(8);
  begin("fin_clipped_empty", 8);
  syn(); seg(0, 8); seg(7, 3, 0, true); pop(8); seg(8, 2); pop(8);
  begin("data_after_fin", 64);
  syn(); seg(4, 2, 0, true); seg(6, 4); seg(5, 4, 1); seg(0, 4); pop(64);
  begin("data_after_close", 64);
  syn(); seg(0, 4, 0, true); seg(4, 4); seg(0, 4, 1); pop(2); seg(2, 8); pop(64);

  begin("syn_with_data", 64);
  syn(pay(0, 6)); seg(6, 3); pop(64);
  begin("syn_fin", 64);
  syn("", true); seg(0, 3); pop(64);
  begin("syn_fin_data", 64);
  syn(pay(0, 4), true); pop(64);
  begin("second_syn", 64);
  syn(pay(0, 3)); raw(77777u, pay(0, 5, 1), true); seg(5, 2); raw(g_isn + 9u, pay(20, 2, 2), true); pop(64);
  begin("data_before_syn", 64);
  seg(0, 4); raw(5u, pay(9, 3)); syn(); seg(0, 4); pop(64);
  begin("fin_before_syn", 64);
  seg(0, 0, 0, true); syn(); seg(0, 2); pop(64);

  begin("rst_first", 64);
  raw(g_isn, "", false, false, true); syn(); seg(0, 4); pop(64);
  begin("rst_syn_first", 64);
  raw(g_isn, pay(0, 3), true, false, true); syn(); seg(0, 4);
  begin("rst_middle", 64);
  syn(); seg(0, 4); seg(8, 4); raw(g_isn + 5u, pay(4, 4), false, false, true); seg(4, 4); pop(3); pop(64);
  begin("set_error_then_data", 64);
  syn(); seg(0, 4); set_error(); seg(4, 4); raw(g_isn, "", true); pop(64);

  for (uint32_t isn : {0u, 0x80000000u, 0xFFFFFFFFu}) {
    begin("isn_" + std::to_string(isn), 64, isn);
    syn(); seg(0, 5); seg(7, 3); seg(5, 2); pop(64); seg(10, 4, 0, true); pop(64);
  }
  begin("cross_2_32", 100, 0xFFFFFF00u);
  syn();
  for (uint64_t at = 0; at < 600; at += 60) {
    seg(at + 30, 30); seg(at, 30); pop(60);
  }
  seg(600, 5, 0, true); pop(64);

  // seqnos around half the sequence space away from the checkpoint (pushed + 1)
  for (int pushed : {0, 40}) {
    for (uint32_t d : {0x7FFFFFFFu, 0x80000000u, 0x80000001u}) {
      for (int side = 0; side < 2; ++side) {
        begin(std::string("half_space_") + (side ? "below_" : "above_") + std::to_string(d) + "_pushed" +
                  std::to_string(pushed),
              64, 5000);
        syn();
        if (pushed) { seg(0, 40); pop(40); }
        const uint32_t ck = g_isn + uint32_t(pushed) + 1u;
        raw(side ? ck - d : ck + d, pay(3, 4, 1));
        raw(side ? ck - d : ck + d, pay(3, 4, 2), false, true);
        seg(pushed, 6); pop(64);
      }
    }
  }
  begin("seqno_is_isn_no_syn", 64);
  syn(); raw(g_isn, pay(0, 4, 1)); raw(g_isn, pay(0, 4, 1), false, true); seg(0, 4); pop(64);
  begin("seqno_below_isn", 64);
  syn(); raw(g_isn - 1u, pay(0, 4, 1)); raw(g_isn - 200u, pay(0, 4, 2), false, true); seg(0, 4); pop(64);
}

std::string hex(const std::string& s) {
  static const char* d = "0123456789abcdef";
  std::string o;
  for (unsigned char c : s) { o += d[c >> 4]; o += d[c & 15]; }
  return o;
}

uint32_t raw_of(const Wrap32& w) { return uint32_t(w.unwrap(Wrap32{0}, 0)); }

}  // namespace

int main() {
  build();
  std::printf("{\"scenarios\": [\n");
  for (size_t si = 0; si < g_all.size(); ++si) {
    const Scenario& sc = g_all[si];
    TCPReceiver rx{Reassembler{ByteStream{sc.capacity}}};
    std::printf(" {\"tag\": \"%s\", \"capacity\": %llu, \"ops\": [\n", sc.tag.c_str(), (unsigned long long)sc.capacity);
    for (size_t k = 0; k < sc.ops.size(); ++k) {
      const Op& o = sc.ops[k];
      std::printf("  {");
      if (o.kind == 0) {
        TCPSenderMessage m;
        m.seqno = Wrap32{o.seqno}, m.SYN = o.syn, m.FIN = o.fin, m.RST = o.rst, m.payload = o.payload;
        rx.receive(m);
        std::printf("\"op\": \"recv\", \"seqno\": %u, \"syn\": %d, \"fin\": %d, \"rst\": %d, \"payload\": \"%s\"", o.seqno,
                    int(o.syn), int(o.fin), int(o.rst), hex(o.payload).c_str());
      } else if (o.kind == 1) {
        std::string out;
        read(rx.reader(), o.n, out);
        std::printf("\"op\": \"pop\", \"n\": %llu, \"popped\": \"%s\"", (unsigned long long)o.n, hex(out).c_str());
      } else {
        rx.reader().set_error();
        std::printf("\"op\": \"set_error\"");
      }
      const TCPReceiverMessage s = rx.send();
      std::printf(", \"pushed\": %llu, \"pending\": %llu, \"avail\": %llu, \"closed\": %d, \"error\": %d, ",
                  (unsigned long long)rx.writer().bytes_pushed(), (unsigned long long)rx.reassembler().bytes_pending(),
                  (unsigned long long)rx.writer().available_capacity(), int(rx.writer().is_closed()),
                  int(rx.writer().has_error()));
      if (s.ackno.has_value())
        std::printf("\"ackno\": %u", raw_of(*s.ackno));
      else
        std::printf("\"ackno\": null");
      std::printf(", \"window\": %u, \"rst\": %d}%s\n", unsigned(s.window_size), int(s.RST),
                  k + 1 < sc.ops.size() ? "," : "");
    }
    std::printf(" ]}%s\n", si + 1 < g_all.size() ? "," : "");
  }
  std::printf("]}\n");
  return 0;
}
