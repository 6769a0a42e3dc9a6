// unwrap_selftest.cpp — icsum_unwrap.cpp linked alone (no HIP, no context),
// built with ASan + UBSan by tests/test_unwrap_records.py and run as a child
// process.  For every length 0..130, every header length in {5, 6, 15} and
// data offset in {4, 5, 6, 15}, a datagram whose checksums verify is cut to
// that length, its checksums fixed again, and copied to the END of an exactly
// sized heap block at start alignments +0..+3: a read past the datagram trips
// the sanitizer.  The record must say PARSED exactly when the header and 20
// bytes of TCP fit and the data offset is at least 5, hold the fields that
// were put on the wire, and be zero otherwise.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "icsum.h"

namespace {

int failures = 0;
#define EXPECT(c)                                                                  \
  do {                                                                             \
    if (!(c)) {                                                                    \
      if (++failures <= 20) std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
    }                                                                              \
  } while (0)

uint32_t g_state = 0x1071;
uint8_t next_byte() {
  g_state = g_state * 1664525u + 1013904223u;
  return uint8_t(g_state >> 16);
}

uint32_t fold(uint32_t s) {
  while (s > 0xffffu) s = (s >> 16) + (s & 0xffffu);
  return ~s & 0xffffu;
}

void set16(std::vector<uint8_t>& b, size_t at, uint32_t v) {
  b[at] = uint8_t(v >> 8);
  b[at + 1] = uint8_t(v);
}

struct Fields {
  uint32_t src, dst, seqno, ackno;
  uint16_t sport, dport, window, id;
  uint8_t flags, ttl;
};

// `len` bytes of a datagram with `hlen` header words and data offset `doff`,
// both checksums valid over what is there (the TCP one only when its field is)
std::vector<uint8_t> make(size_t len, uint32_t hlen, uint32_t doff, const Fields& f) {
  std::vector<uint8_t> b(4 * hlen + 4 * 15 + 64);
  for (auto& c : b) c = next_byte();
  b[0] = uint8_t(0x40 | hlen);
  set16(b, 4, f.id);
  b[8] = f.ttl;
  b[9] = 6;
  set16(b, 12, f.src >> 16);
  set16(b, 14, f.src & 0xffffu);
  set16(b, 16, f.dst >> 16);
  set16(b, 18, f.dst & 0xffffu);
  const size_t t = 4 * hlen;
  set16(b, t, f.sport);
  set16(b, t + 2, f.dport);
  set16(b, t + 4, f.seqno >> 16);
  set16(b, t + 6, f.seqno & 0xffffu);
  set16(b, t + 8, f.ackno >> 16);
  set16(b, t + 10, f.ackno & 0xffffu);
  b[t + 12] = uint8_t(doff << 4 | (next_byte() & 0x0f));
  b[t + 13] = f.flags;
  set16(b, t + 14, f.window);
  b.resize(len);
  if (len >= 4) set16(b, 2, uint32_t(len));
  if (len >= t + 18) {
    set16(b, t + 16, 0);
    uint32_t s = (f.src >> 16) + (f.src & 0xffffu) + (f.dst >> 16) + (f.dst & 0xffffu) + 6 +
                 ((uint32_t(len) - 4 * hlen) & 0xffffu);
    for (size_t k = t; k < len; ++k) s += ((k - t) & 1) ? b[k] : uint32_t(b[k]) << 8;
    set16(b, t + 16, fold(s));
  }
  if (len >= 20) {
    set16(b, 10, 0);
    uint32_t s = 0;
    for (size_t k = 0; k < 20; k += 2) s += ((uint32_t(b[k]) << 8) | b[k + 1]) & (k == 6 ? 0x7fffu : 0xffffu);
    set16(b, 10, fold(s));
  }
  return b;
}

}  // namespace

int main() {
  size_t runs = 0, parsed = 0;
  for (size_t len = 0; len <= 130; ++len)
    for (uint32_t hlen : {5u, 6u, 15u})
      for (uint32_t doff : {4u, 5u, 6u, 15u}) {
        Fields f{};
        f.src = uint32_t(next_byte()) << 24 | uint32_t(next_byte()) << 8 | next_byte();
        f.dst = ~f.src;
        f.seqno = 0xfffffff0u + next_byte();
        f.ackno = 0x80000000u | next_byte();
        f.sport = uint16_t(next_byte() << 8 | next_byte());
        f.dport = uint16_t(~f.sport);
        f.window = uint16_t(next_byte() << 8);
        f.id = uint16_t(0xff00u | next_byte());
        f.flags = next_byte();
        f.ttl = next_byte();
        const std::vector<uint8_t> d = make(len, hlen, doff, f);
        for (size_t a = 0; a < 4; ++a) {
          // operator new[] returns 16-byte aligned storage: the datagram starts at +a and ends at the block's end
          uint8_t* block = new uint8_t[a + len];
          if (len) std::memcpy(block + a, d.data(), len);
          ics_tcp_rx r;
          std::memset(&r, 0xa5, sizeof r);
          EXPECT(ics_tcp_unwrap_one(block + a, len, &r) == ICS_OK);
          delete[] block;
          ++runs;
          const bool want = 4 * hlen + 20 <= len && doff >= 5;
          const bool got = (r.status & 7u) == 7u;
          EXPECT(got == want);
          EXPECT(r.reserved[0] == 0 && r.reserved[1] == 0 && r.reserved[2] == 0 && r.msg.reserved == 0);
          if (len >= 20) EXPECT((r.status & ICS_ST_IPV4_OK) && (r.status & ICS_ST_PROTO_TCP));
          if (len < 20) EXPECT(r.status == 0);
          if (len >= 4 * hlen + 18) EXPECT(r.status & ICS_ST_TCP_CKSUM_OK);
          if (!got) {
            ics_tcp_rx z;
            std::memset(&z, 0, sizeof z);
            z.status = r.status;
            EXPECT(std::memcmp(&r, &z, sizeof r) == 0);
            continue;
          }
          ++parsed;
          const bool ack = (f.flags & ICS_TCP_ACK) != 0;
          EXPECT(r.msg.src == f.src && r.msg.dst == f.dst && r.msg.seqno == f.seqno);
          EXPECT(r.msg.ackno == (ack ? f.ackno : 0u));
          EXPECT(r.msg.src_port == f.sport && r.msg.dst_port == f.dport && r.msg.window == f.window);
          EXPECT(r.msg.flags == (f.flags & 0x17u) && r.msg.ttl == f.ttl && r.msg.id == f.id);
          const size_t po = 4 * hlen + 4 * doff;
          EXPECT(r.pay_off == (po < len ? po : len));
          EXPECT(size_t(r.pay_off) + r.pay_len == len);
        }
      }
  // argument errors (linked alone there is no message store: the code is the whole answer)
  ics_tcp_rx r;
  uint8_t one = 0;
  EXPECT(ics_tcp_unwrap_one(&one, 1, nullptr) == ICS_ERR_INVALID);
  EXPECT(ics_tcp_unwrap_one(nullptr, 1, &r) == ICS_ERR_INVALID);
  EXPECT(ics_tcp_unwrap_one(nullptr, 0, &r) == ICS_OK && r.status == 0);
  EXPECT(parsed > runs / 4);
  if (failures) {
    std::fprintf(stderr, "unwrap_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("unwrap_selftest ok: %zu runs, %zu parsed\n", runs, parsed);
  return 0;
}
