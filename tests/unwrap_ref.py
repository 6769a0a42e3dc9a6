"""ics_tcp_rx (include/icsum.h) restated in Python: what the reference's
IPv4Header::parse (util/ipv4_header/ipv4_header.cpp:9-59), TCPSegment::parse
(util/tcp_segment/tcp_segment.cpp:9-66) and TCPOverIPv4Adapter::unwrap_tcp_in_ip
(util/tcp_over_ip/tcp_over_ip.cpp:10-67) read out of one datagram's bytes.

  verify_status()  the ICS_ST_* byte ICS_MODE_VERIFY writes
  unwrap()         the 40-byte record, packed as the C struct lies in memory
  fields()         a packed record as a dict
  RefAdapter       the adapter's gates applied from record fields alone
  canonical()      the round-trip conditions, checked from the bytes
  wrap40()         the 40 header bytes wrap_tcp_in_ip serializes for a record

The restatement is checked against the real reference's parses in
test_unwrap_records.py (tests/golden/unwrap_cases.json,
tools/gen_unwrap_golden.cpp); the device is then checked against it."""
import json
import os
import struct

ST_IPV4_OK, ST_TCP_CKSUM_OK, ST_TCP_HDR_OK, ST_PROTO_TCP = 0x01, 0x02, 0x04, 0x08
PARSED = 0x07
TCP_FIN, TCP_SYN, TCP_RST, TCP_ACK = 0x01, 0x02, 0x04, 0x10
REC = struct.Struct("<IIIIHHHBBHHIIB3x")  # ics_tcp_msg, pay_off, pay_len, status, reserved[3]
assert REC.size == 40
NAMES = ("src", "dst", "seqno", "ackno", "src_port", "dst_port", "window", "flags", "ttl", "id", "reserved",
         "pay_off", "pay_len", "status")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unwrap_cases.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def fold(s):
    """InternetChecksum::value() of a uint32 sum_ (util/tools/checksum.h:31-41)"""
    s &= 0xFFFFFFFF
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def header_checksum(d):
    """IPv4Header::compute_checksum (ipv4_header.cpp:113-123) from the wire's
    20 fixed bytes: checksum field zero, the reserved flag bit dropped, options
    never summed"""
    s = 0
    for k in range(0, 20, 2):
        w = d[k] << 8 | d[k + 1]
        if k == 6:
            w &= 0x7FFF
        if k == 10:
            w = 0
        s += w
    return fold(s)


def tcp_offset(d):
    """where the bytes behind the IPv4 header start: 4 * hlen clamped to [20, len]"""
    return min(max(4 * (d[0] & 15), 20), len(d))


def verify_status(d):
    d = bytes(d)
    if len(d) < 20:
        return 0
    hlen = d[0] & 15
    off = tcp_offset(d)
    t = d[off:]
    be16 = lambda k: d[k] << 8 | d[k + 1]  # noqa: E731
    # pseudo_checksum (ipv4_header.cpp:103-110), payload_length() mod 2^16, then add() over every byte
    s = be16(12) + be16(14) + be16(16) + be16(18) + d[9] + ((be16(2) - 4 * hlen) & 0xFFFF)
    s += 256 * sum(t[0::2]) + sum(t[1::2])
    st = 0
    if d[0] >> 4 == 4 and hlen >= 5 and header_checksum(d) == be16(10):
        st |= ST_IPV4_OK
    if fold(s) == 0:
        st |= ST_TCP_CKSUM_OK
    if len(t) >= 20 and t[12] >> 4 >= 5:
        st |= ST_TCP_HDR_OK
    if d[9] == 6:
        st |= ST_PROTO_TCP
    return st


def unwrap(d):
    """the packed 40-byte ics_tcp_rx of one datagram"""
    d = bytes(d)
    st = verify_status(d)
    if st & PARSED != PARSED:
        return REC.pack(*([0] * 13), st)
    hl = 4 * (d[0] & 15)
    t = d[hl:]
    assert len(t) >= 20  # TCP_HDR_OK
    be = lambda b: int.from_bytes(b, "big")  # noqa: E731
    flags = t[13]
    pay_off = min(hl + 4 * (t[12] >> 4), len(d))
    return REC.pack(be(d[12:16]), be(d[16:20]), be(t[4:8]), be(t[8:12]) if flags & TCP_ACK else 0, be(t[0:2]),
                    be(t[2:4]), be(t[14:16]), flags & 0x17, d[8], be(d[4:6]), 0, pay_off,
                    (len(d) - pay_off) & 0xFFFFFFFF, st)


def fields(rec):
    return dict(zip(NAMES, REC.unpack(bytes(rec))))


class RefAdapter:
    """tcp_over_ip.cpp:14-64 from record fields: `source` / `destination` are
    (host-order ip, port).  accept() is sequential: a listening adapter's first
    clean SYN to its port rewrites both endpoints and ends listening."""

    def __init__(self, listening, source, destination):
        self.listening = bool(listening)
        self.source = tuple(source)
        self.destination = tuple(destination)

    def accept(self, rec):
        r = rec if isinstance(rec, dict) else fields(rec)
        if not self.listening and (r["dst"] != self.source[0] or r["src"] != self.destination[0]):
            return False
        if not r["status"] & ST_PROTO_TCP:
            return False
        if r["status"] & PARSED != PARSED:  # IPv4Header::parse or TCPSegment::parse failed
            return False
        if r["dst_port"] != self.source[1]:
            return False
        if self.listening:
            if not r["flags"] & TCP_SYN or r["flags"] & TCP_RST:
                return False
            self.source = (r["dst"], self.source[1])
            self.destination = (r["src"], r["src_port"])
            self.listening = False
        return r["src_port"] == self.destination[1]


def make_dgram(rng, n, hlen=5, doff=5, fix=0.85, flip=0.08):
    """`n` random bytes (`rng`: random.Random) shaped as a datagram with `hlen`
    header words and data offset `doff` where those bytes exist; with
    probability `fix` both checksums are made to verify, with `flip` one bit is
    then inverted somewhere"""
    d = bytearray(rng.randbytes(n))
    if n < 20:
        return bytes(d)
    d[0] = 0x40 | hlen if rng.random() < 0.95 else rng.randrange(256)
    d[9] = 6 if rng.random() < 0.85 else 17
    d[2:4] = (n & 0xFFFF).to_bytes(2, "big")
    t = min(max(4 * hlen, 20), n)
    if n - t >= 14:
        d[t + 12] = (doff << 4) | rng.randrange(16)
        d[t + 13] = rng.choice([0x00, 0x10, 0x02, 0x12, 0x11, 0x04, 0x18, 0xFF, rng.randrange(256)])
    if rng.random() < fix:
        if n - t >= 18:
            d[t + 16:t + 18] = b"\0\0"
            s = sum(d[12:20:2]) * 256 + sum(d[13:20:2]) + d[9] + ((n - 4 * (d[0] & 15)) & 0xFFFF)
            s += 256 * sum(d[t::2]) + sum(d[t + 1::2])
            d[t + 16:t + 18] = fold(s).to_bytes(2, "big")
        d[10:12] = header_checksum(d).to_bytes(2, "big")
    if rng.random() < flip:
        d[rng.randrange(n)] ^= 1 << rng.randrange(8)
    return bytes(d)


def canonical(d):
    """the round-trip conditions of include/icsum.h, from the bytes: what
    wrap_tcp_in_ip can have produced (hlen 5, tos 0, DF only, len == length mod
    2^16, data offset 5, urgent 0, no flag bits outside 0x17) and parses"""
    d = bytes(d)
    return (len(d) >= 40 and d[0] == 0x45 and d[1] == 0 and d[6:8] == b"\x40\x00"
            and (d[2] << 8 | d[3]) == len(d) & 0xFFFF and d[32] >> 4 == 5 and d[38:40] == b"\x00\x00"
            and d[33] & ~0x17 == 0 and d[9] == 6 and verify_status(d) & PARSED == PARSED)


def wrap40(rec, payload):
    """serialize(wrap_tcp_in_ip(msg))'s first 40 bytes (ipv4_header.cpp:62-86,
    tcp_segment.cpp:76-118) from a record's msg and the payload bytes"""
    r = rec if isinstance(rec, dict) else fields(rec)
    payload = bytes(payload)
    total = (40 + len(payload)) & 0xFFFF
    ip = bytearray(struct.pack(">BBHHHBBHII", 0x45, 0, total, r["id"], 0x4000, r["ttl"], 6, 0, r["src"], r["dst"]))
    tcp = bytearray(struct.pack(">HHIIBBHHH", r["src_port"], r["dst_port"], r["seqno"], r["ackno"], 0x50, r["flags"],
                                r["window"], 0, 0))
    s = (r["src"] >> 16) + (r["src"] & 0xFFFF) + (r["dst"] >> 16) + (r["dst"] & 0xFFFF) + 6 + ((total - 20) & 0xFFFF)
    body = bytes(tcp) + payload
    s += 256 * sum(body[0::2]) + sum(body[1::2])
    tcp[16:18] = fold(s).to_bytes(2, "big")
    ip[10:12] = header_checksum(ip).to_bytes(2, "big")
    return bytes(ip) + bytes(tcp)
