// icsum_unwrap.cpp — ics_tcp_unwrap_one (include/icsum.h): the host
// restatement of the record k_tcp_unwrap writes (kernels/icsum_unwrap.h) and
// of the ICS_MODE_VERIFY status byte behind it, for one datagram.  Plain C++:
// no HIP, no context, usable (and tested) on a machine without a GPU; it links
// alone.
//
// Reference semantics kept: IPv4Header::parse (util/ipv4_header/ipv4_header.cpp:9-59:
// version 4, hlen >= 5, the checksum recomputed over the 20 serialized bytes
// with the reserved flag bit dropped, options skipped and never summed),
// pseudo_checksum (:103-110, payload_length wrapping mod 2^16),
// TCPSegment::parse (util/tcp_segment/tcp_segment.cpp:11-18 the sum over every
// byte behind the IPv4 header, :25-65 the fields, an absent ackno reset to 0,
// options removed with Parser::remove_prefix, which stops at the end).
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "icsum.h"

namespace icsum::detail {
// icsum_api.cpp's error reporting; absent (null) when this file is linked alone
int fail(int code, const char* fmt, ...) __attribute__((weak, format(printf, 2, 3)));
}  // namespace icsum::detail

namespace {

#define UNWRAP_FAIL(code, ...) (::icsum::detail::fail ? ::icsum::detail::fail((code), __VA_ARGS__) : (code))

static_assert(sizeof(ics_tcp_msg) == 28 && sizeof(ics_tcp_rx) == 40 && offsetof(ics_tcp_rx, pay_off) == 28 &&
                  offsetof(ics_tcp_rx, status) == 36,
              "ics_tcp_rx layout");

inline uint32_t be16(const uint8_t* p) { return (uint32_t(p[0]) << 8) | p[1]; }
inline uint32_t be32(const uint8_t* p) { return (be16(p) << 16) | be16(p + 2); }

// InternetChecksum::value() (util/tools/checksum.h:31-41)
inline uint32_t fold_value(uint32_t s) {
  while (s > 0xffffu) s = (s >> 16) + (s & 0xffffu);
  return ~s & 0xffffu;
}

// the ICS_MODE_VERIFY status byte of one datagram of >= 20 bytes; *t_off: where
// its TCP part starts (4 * hlen clamped to [20, len], ipv4_header.cpp:50)
uint8_t verify_status(const uint8_t* d, size_t len, size_t* t_off) {
  const uint32_t ver = d[0] >> 4, hlen = d[0] & 0x0fu;
  // compute_checksum (ipv4_header.cpp:113-123): cksum = 0, reserved flag bit dropped
  uint32_t hs = 0;
  for (int k = 0; k < 20; k += 2) {
    uint32_t w = be16(d + k);
    if (k == 6) w &= 0x7fffu;
    if (k == 10) w = 0;
    hs += w;
  }
  const uint32_t ipc = fold_value(hs);
  size_t off = 4u * hlen;
  if (off < 20) off = 20;
  if (off > len) off = len;
  *t_off = off;
  const size_t rem = len - off;
  const uint32_t src = be32(d + 12), dst = be32(d + 16);
  // pseudo_checksum (ipv4_header.cpp:103-110)
  uint32_t sum = (src >> 16) + (src & 0xffffu) + (dst >> 16) + (dst & 0xffffu) + d[9] +
                 ((be16(d + 2) - 4u * hlen) & 0xffffu);
  // InternetChecksum::add over every byte behind the header (checksum.h:20-28), a uint32 that wraps
  for (size_t k = 0; k < rem; ++k) sum += (k & 1u) ? uint32_t(d[off + k]) : uint32_t(d[off + k]) << 8;
  uint8_t st = 0;
  if (ver == 4 && hlen >= 5 && ipc == be16(d + 10)) st |= ICS_ST_IPV4_OK;
  if (fold_value(sum) == 0) st |= ICS_ST_TCP_CKSUM_OK;
  if (rem >= 20 && (d[off + 12] >> 4) >= 5) st |= ICS_ST_TCP_HDR_OK;
  if (d[9] == 6) st |= ICS_ST_PROTO_TCP;
  return st;
}

}  // namespace

extern "C" int ics_tcp_unwrap_one(const void* dgram, size_t len, ics_tcp_rx* out) {
  if (!out) return UNWRAP_FAIL(ICS_ERR_INVALID, "null record");
  if (!dgram && len) return UNWRAP_FAIL(ICS_ERR_INVALID, "null datagram of %zu bytes", len);
  std::memset(out, 0, sizeof *out);
  if (len < 20) return ICS_OK;  // ics_ipv4_tcp_batch: status 0
  const uint8_t* d = static_cast<const uint8_t*>(dgram);
  size_t hl = 0;
  out->status = verify_status(d, len, &hl);
  if ((out->status & 7u) != 7u) return ICS_OK;
  // PARSED: hlen >= 5, so hl = 4 * hlen, and hl + 20 <= len
  const uint8_t* t = d + hl;
  ics_tcp_msg& m = out->msg;
  m.src = be32(d + 12);
  m.dst = be32(d + 16);
  m.ttl = d[8];
  m.id = uint16_t(be16(d + 4));
  m.src_port = uint16_t(be16(t));
  m.dst_port = uint16_t(be16(t + 2));
  m.seqno = be32(t + 4);
  m.ackno = (t[13] & ICS_TCP_ACK) ? be32(t + 8) : 0u;  // tcp_segment.cpp:42-45
  m.flags = uint8_t(t[13] & 0x17u);
  m.window = uint16_t(be16(t + 14));
  const size_t po = hl + 4u * (t[12] >> 4);  // options removed, stopping at the end (parser.h:54-68)
  out->pay_off = uint32_t(po < len ? po : len);
  out->pay_len = uint32_t(len - out->pay_off);
  return ICS_OK;
}
