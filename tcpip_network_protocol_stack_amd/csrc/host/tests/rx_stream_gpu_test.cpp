// rx_stream_gpu_test.cpp — BatchEngine::receive_records (message records and
// the copy into the stream's ring on the device, the adapter's gates from
// record fields) against the same wires taken one by one on the host: the
// per-object unwrap_tcp_in_ip decides which datagrams count, ics_tcp_unwrap_one
// gives their records, and a host-only icsum::RxStream plans them with the
// pieces applied to a ring in host memory.  Batch for batch the `take` arrays,
// every stat, send() and the bytes read are equal, and the bytes read are the
// stream the peer sent.  Exit 0 = identical.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "batch.h"
#include "icsum.h"

namespace {
int failures = 0;
#define EXPECT(c)                                                     \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                               \
        }                                                             \
    } while (0)

std::string joined(const std::vector<std::string>& v)
{
    std::string r;
    for (auto& s : v) r += s;
    return r;
}

struct Endpoints
{
    const char* src;
    uint16_t sport;
    const char* dst;
    uint16_t dport;
};

void* device_alloc(icsum::BatchEngine& eng, size_t bytes)
{
    void* d = nullptr;
    if (ics_malloc(eng.context(), &d, bytes) != ICS_OK) throw std::runtime_error(ics_last_error());
    return d;
}

void to_device(icsum::BatchEngine& eng, void* d, const void* h, size_t bytes)
{
    if (ics_memcpy_htod(eng.context(), d, h, bytes, nullptr) != ICS_OK ||
        ics_stream_synchronize(eng.context(), nullptr) != ICS_OK)
        throw std::runtime_error(ics_last_error());
}

std::string wire_of(const Endpoints& e, const TCPMessage& m)
{
    TCPOverIPv4Adapter a;
    a.config_mut().source = Address{e.src, e.sport};
    a.config_mut().destination = Address{e.dst, e.dport};
    return joined(serialize(a.wrap_tcp_in_ip(m)));
}

char stream_byte(uint64_t i) { return static_cast<char>((i * 131 + (i >> 8) * 17 + 7) & 0xff); }

bool same_stats(const ics_rx_stats_t& a, const ics_rx_stats_t& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
}  // namespace

int main()
{
    icsum::BatchEngine eng(0);
    std::mt19937_64 rng(0x72787374);
    constexpr uint64_t kCap = 4096;
    constexpr uint32_t kIsn = 0xFFFFF000u;  // the stream crosses 2^32 in sequence space
    const Endpoints peer{"10.9.8.7", 80, "10.1.2.3", 4321};
    const Endpoints stranger{"10.9.8.9", 80, "10.1.2.3", 4321};

    TCPOverIPv4Adapter a_dev, a_obj;  // listening: the peer's SYN connects both
    for (TCPOverIPv4Adapter* a : {&a_dev, &a_obj}) {
        a->config_mut().source = Address{"0", 4321};
        a->set_listening(true);
    }
    icsum::RxStream rx_dev(eng, kCap), rx_host(kCap);
    std::vector<uint8_t> ring(kCap, 0x5a);
    uint64_t read_total = 0, accepted_total = 0, batches = 0;
    bool fin_sent = false;

    for (int round = 0; round < 40 && !rx_host.stats().closed; ++round) {
        const uint64_t pushed = rx_host.stats().bytes_pushed;
        std::vector<std::string> wires;
        for (int k = 0; k < 300; ++k) {
            TCPMessage m;
            const unsigned kind = rng() % 16;
            if (round == 0 && k == 3) {
                m.sender.SYN = true;
                m.sender.seqno = Wrap32{kIsn};
            } else {
                // around the window: behind the first unassembled byte, at it, ahead of it, past the edge
                const int64_t idx = kind < 5 ? static_cast<int64_t>(pushed) + static_cast<int64_t>(rng() % 1500) - 300
                                             : static_cast<int64_t>(pushed) + static_cast<int64_t>(rng() % (kCap + 600)) - 300;
                const size_t len = rng() % 1001;
                m.sender.seqno = Wrap32{kIsn + 1u + static_cast<uint32_t>(idx)};
                m.sender.payload.resize(len);
                for (size_t b = 0; b < len; ++b) m.sender.payload[b] = stream_byte(static_cast<uint64_t>(idx + static_cast<int64_t>(b)));
                if (round == 30 && k == 299 && idx >= 0) m.sender.FIN = fin_sent = true;
            }
            if (rng() % 3) m.receiver.ackno = Wrap32{static_cast<uint32_t>(rng())};
            std::string w = wire_of(kind == 15 ? stranger : peer, m);
            if (rng() % 11 == 0) w[rng() % w.size()] ^= static_cast<char>(1u << (rng() % 8));  // fails a checksum (mostly)
            wires.push_back(std::move(w));
        }
        std::string arena;
        std::vector<uint64_t> off{0};
        for (auto& w : wires) {
            arena += w;
            off.push_back(arena.size());
        }
        const size_t n = wires.size();
        // the device path
        void* d = device_alloc(eng, arena.size());
        to_device(eng, d, arena.data(), arena.size());
        std::vector<uint8_t> take_dev(n, 7);
        const size_t acc = eng.receive_records(a_dev, rx_dev, d, off.data(), n, take_dev.data());
        // the host path: per-object gates, records of one datagram each, plan, pieces applied here
        std::vector<uint8_t> take(n, 0);
        std::vector<ics_tcp_rx> recs(n);
        for (size_t i = 0; i < n; ++i) {
            InternetDatagram dg;
            if (parse(dg, std::vector<std::string>{wires[i]})) take[i] = a_obj.unwrap_tcp_in_ip(dg).has_value();
            EXPECT(ics_tcp_unwrap_one(wires[i].data(), wires[i].size(), &recs[i]) == ICS_OK);
        }
        EXPECT(take == take_dev);
        EXPECT(acc == static_cast<size_t>(std::count(take.begin(), take.end(), 1)));
        for (const ics_copy_piece& p : rx_host.plan(recs, take.data(), off.data()))
            std::memcpy(ring.data() + p.dst, arena.data() + p.src, p.len);
        EXPECT(same_stats(rx_dev.stats(), rx_host.stats()));
        const TCPReceiverMessage s1 = rx_dev.send(), s2 = rx_host.send();
        EXPECT(s1.ackno == s2.ackno && s1.window_size == s2.window_size && s1.RST == s2.RST);
        // read what is buffered (sometimes only a part of it) on both sides
        const uint64_t have = rx_host.stats().bytes_buffered, want = rng() % 4 ? have : have / 2;
        const std::string got = rx_dev.read(want);
        std::string host;
        for (auto [o, l] : rx_host.peek()) host.append(reinterpret_cast<const char*>(ring.data()) + o, l);
        host.resize(static_cast<size_t>(want));
        rx_host.pop(want);
        EXPECT(got == host);
        for (size_t b = 0; b < host.size(); ++b)
            if (host[b] != stream_byte(read_total + b)) {
                EXPECT(!"the stream the peer sent");
                break;
            }
        read_total += want;
        accepted_total += acc;
        ++batches;
        EXPECT(same_stats(rx_dev.stats(), rx_host.stats()));
        ics_free(eng.context(), d);  // synchronises: the copy has run
    }
    EXPECT(a_dev.listening() == a_obj.listening() && !a_dev.listening());
    EXPECT(read_total > 8 * kCap);  // the ring wrapped
    EXPECT(accepted_total > 3000);
    // an empty batch, and a host-only stream refused by the device call
    EXPECT(eng.receive_records(a_dev, rx_dev, nullptr, nullptr, 0) == 0);
    bool threw = false;
    try {
        const uint64_t off1[2] = {0, 40};
        void* d = device_alloc(eng, 64);
        try {
            eng.receive_records(a_dev, rx_host, d, off1, 1);
        } catch (const std::exception& e) {
            threw = std::strstr(e.what(), "without a ring") != nullptr;
        }
        ics_free(eng.context(), d);
    } catch (const std::exception&) {
    }
    EXPECT(threw);
    std::printf("%s: receive_records == per-object gates + host plan (%llu batches, %llu accepted, %llu bytes read, fin %d)\n",
                failures ? "FAILED" : "OK", (unsigned long long)batches, (unsigned long long)accepted_total,
                (unsigned long long)read_total, int(fin_sent));
    return failures ? 1 : 0;
}
