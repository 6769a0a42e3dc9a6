// rx_stream_test.cpp — icsum::RxStream::plan against the reference's own
// TCPReceiver (src/tcp_receiver, src/reassembler, src/byte_stream,
// src/wrapping_integers: read-only, compiled in place on the drop-in headers,
// as dropin_stack is), segment for segment.  6000 mixed wires — the peer's
// segments around the window in any order, overlapping, a fifth of the
// overlaps with different bytes, SYNs, FINs, an RST near the end, strangers
// and corrupted datagrams — go through the per-object unwrap_tcp_in_ip; every
// accepted message is received by the reference and, as its ics_tcp_unwrap_one
// record, planned by the RxStream with the pieces applied to a ring here.
// After every segment: bytes_pushed, bytes_pending, available capacity,
// closed, error and send(); after every read the same bytes.  CPU only; built
// where the reference sources exist.  Exit 0 = identical.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "batch.h"
#include "icsum.h"
#include "tcp_receiver.h"

namespace {
int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            if (++failures <= 20) std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                             \
    } while (0)

std::string joined(const std::vector<std::string>& v)
{
    std::string r;
    for (auto& s : v) r += s;
    return r;
}

char stream_byte(uint64_t i, unsigned salt) { return static_cast<char>((i * 131 + (i >> 8) * 17 + 7 + salt * 89) & 0xff); }
}  // namespace

int main()
{
    std::mt19937_64 rng(0x72656173);
    size_t accepted = 0, reads = 0, read_bytes = 0, wires_total = 0;
    for (const uint64_t cap : {uint64_t{7}, uint64_t{1000}, uint64_t{65535}}) {
        const uint32_t isn = cap == 7 ? 0u : cap == 1000 ? 0xFFFFFF00u : 0x80000000u;
        TCPReceiver ref{Reassembler{ByteStream{cap}}};
        icsum::RxStream rx(cap);
        std::vector<uint8_t> ring(cap, 0x5a);
        TCPOverIPv4Adapter to_wire, adapter;  // the peer's side, ours
        to_wire.config_mut().source = Address{"10.9.8.7", 80};
        to_wire.config_mut().destination = Address{"10.1.2.3", 4321};
        adapter.config_mut().source = Address{"10.1.2.3", 4321};
        adapter.config_mut().destination = Address{"10.9.8.7", 80};
        const uint64_t maxlen = std::min<uint64_t>(cap / 3 + 1, 1000);
        for (int k = 0; k < 2000; ++k, ++wires_total) {
            const uint64_t pushed = ref.writer().bytes_pushed(), popped = ref.reader().bytes_popped();
            TCPMessage m;
            const unsigned kind = rng() % 20;
            if (k == 2 || kind == 19) {
                m.sender.SYN = true;
                m.sender.seqno = Wrap32{k == 2 ? isn : isn + 99};
            } else {
                const uint64_t len = rng() % (maxlen + 1);
                const int64_t lo = static_cast<int64_t>(pushed) - 2 * static_cast<int64_t>(maxlen);
                const int64_t span = static_cast<int64_t>(popped + cap + maxlen) - lo + 1;
                const int64_t idx = kind < 7 ? static_cast<int64_t>(pushed) - static_cast<int64_t>(rng() % 4)
                                             : lo + static_cast<int64_t>(rng() % static_cast<uint64_t>(span));
                const unsigned salt = rng() % 5 == 0 ? 1 + rng() % 3 : 0;
                m.sender.seqno = Wrap32{isn + 1u + static_cast<uint32_t>(idx)};
                m.sender.payload.resize(len);
                for (uint64_t b = 0; b < len; ++b)
                    m.sender.payload[b] = stream_byte(static_cast<uint64_t>(idx + static_cast<int64_t>(b)), salt);
                m.sender.FIN = k > 1900 && rng() % 30 == 0;
                m.sender.RST = k == 1990;
            }
            std::string w = joined(serialize(to_wire.wrap_tcp_in_ip(m)));
            if (rng() % 9 == 0) w[rng() % w.size()] ^= static_cast<char>(1u << (rng() % 8));
            if (rng() % 13 == 0) w[15] ^= 1;  // another source address (the header checksum then fails too)
            InternetDatagram dg;
            std::optional<TCPMessage> got;
            if (parse(dg, std::vector<std::string>{w})) got = adapter.unwrap_tcp_in_ip(dg);
            ics_tcp_rx rec{};
            EXPECT(ics_tcp_unwrap_one(w.data(), w.size(), &rec) == ICS_OK);
            const uint8_t take = got.has_value();
            if (got) {
                ref.receive(got->sender);
                ++accepted;
            }
            const uint64_t off[2] = {0, w.size()};
            for (const ics_copy_piece& p : rx.plan(std::span<const ics_tcp_rx>(&rec, 1), &take, off))
                std::memcpy(ring.data() + p.dst, w.data() + p.src, p.len);
            const ics_rx_stats_t st = rx.stats();
            EXPECT(st.bytes_pushed == ref.writer().bytes_pushed());
            EXPECT(st.bytes_pending == ref.reassembler().bytes_pending());
            EXPECT(st.available_capacity == ref.writer().available_capacity());
            EXPECT((st.closed != 0) == ref.writer().is_closed() && (st.error != 0) == ref.writer().has_error());
            const TCPReceiverMessage s1 = rx.send(), s2 = ref.send();
            EXPECT(s1.ackno == s2.ackno && s1.window_size == s2.window_size && s1.RST == s2.RST);
            if (rng() % 4 == 0) {
                std::string want, mine;
                read(ref.reader(), rng() % (cap + 2), want);
                for (auto [o, l] : rx.peek()) mine.append(reinterpret_cast<const char*>(ring.data()) + o, l);
                mine.resize(std::min(mine.size(), want.size()));
                EXPECT(mine == want);
                rx.pop(want.size());
                EXPECT(rx.stats().bytes_popped == ref.reader().bytes_popped());
                EXPECT((rx.stats().finished != 0) == ref.reader().is_finished());
                ++reads;
                read_bytes += want.size();
            }
            if (failures) break;
        }
    }
    EXPECT(wires_total == 6000 && accepted > 3000 && read_bytes > 100000);
    std::printf("%s: RxStream::plan == the reference's TCPReceiver (%zu wires, %zu accepted, %zu reads, %zu bytes)\n",
                failures ? "FAILED" : "OK", wires_total, accepted, reads, read_bytes);
    return failures ? 1 : 0;
}
