// unwrap_records_test.cpp — BatchEngine::unwrap_records (the device's message
// records + the adapter's gates from record fields) against unwrap_packed (the
// host field parse) and the per-object unwrap_tcp_in_ip, on the same wires,
// message for message.  Exit 0 = identical.
#include <cstdio>
#include <cstring>
#include <optional>
#include <random>
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

bool same_msg(const TCPMessage& a, const TCPMessage& b)
{
    return a.sender.seqno == b.sender.seqno && a.sender.SYN == b.sender.SYN && a.sender.payload == b.sender.payload &&
           a.sender.FIN == b.sender.FIN && a.sender.RST == b.sender.RST && a.receiver.ackno == b.receiver.ackno &&
           a.receiver.window_size == b.receiver.window_size && a.receiver.RST == b.receiver.RST;
}

struct Endpoints
{
    const char* src;
    uint16_t sport;
    const char* dst;
    uint16_t dport;
};

// serialize(wrap_tcp_in_ip(msg)) from `e.src:sport` to `e.dst:dport`
std::string wire_of(const Endpoints& e, const TCPMessage& m)
{
    TCPOverIPv4Adapter a;
    a.config_mut().source = Address{e.src, e.sport};
    a.config_mut().destination = Address{e.dst, e.dport};
    return joined(serialize(a.wrap_tcp_in_ip(m)));
}

void put16(std::string& w, size_t at, uint32_t v)
{
    w[at] = static_cast<char>(v >> 8);
    w[at + 1] = static_cast<char>(v);
}

// recompute the IPv4 header checksum after an edit of the first 20 bytes
void fix_ip(std::string& w)
{
    put16(w, 10, 0);
    uint32_t s = 0;
    for (size_t k = 0; k < 20; k += 2) s += (static_cast<uint8_t>(w[k]) << 8) | static_cast<uint8_t>(w[k + 1]);
    while (s > 0xffff) s = (s >> 16) + (s & 0xffff);
    put16(w, 10, ~s & 0xffff);
}

struct Run
{
    std::vector<std::string> wires;
    std::vector<uint64_t> off{0};
    std::string arena;
    void push(const std::string& w)
    {
        wires.push_back(w);
        arena += w;
        off.push_back(arena.size());
    }
};

// the three paths over one batch, each on its own copy of the adapter
size_t check_run(icsum::BatchEngine& eng, const Run& r, const TCPOverIPv4Adapter& start, bool end_listening)
{
    TCPOverIPv4Adapter a_rec = start, a_pack = start, a_obj = start;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(r.arena.data());
    const auto rec = eng.unwrap_records(a_rec, bytes, r.off.data(), r.wires.size());
    const auto pack = eng.unwrap_packed(a_pack, bytes, r.off.data(), r.wires.size());
    EXPECT(rec.size() == r.wires.size() && pack.size() == r.wires.size());
    size_t accepted = 0;
    for (size_t i = 0; i < r.wires.size(); ++i) {
        InternetDatagram d;
        std::optional<TCPMessage> want;
        if (parse(d, std::vector<std::string>{r.wires[i]})) want = a_obj.unwrap_tcp_in_ip(d);
        EXPECT(rec[i].has_value() == want.has_value());
        EXPECT(pack[i].has_value() == want.has_value());
        if (want && rec[i]) EXPECT(same_msg(*rec[i], *want));
        if (want && pack[i]) EXPECT(same_msg(*pack[i], *want));
        if (rec[i].has_value() != want.has_value()) std::fprintf(stderr, "  datagram %zu\n", i);
        accepted += want.has_value();
    }
    for (const TCPOverIPv4Adapter* a : {&a_rec, &a_pack}) {
        EXPECT(a->listening() == a_obj.listening());
        EXPECT(a->config().source == a_obj.config().source);
        EXPECT(a->config().destination == a_obj.config().destination);
    }
    EXPECT(a_obj.listening() == end_listening);
    return accepted;
}
}  // namespace

int main()
{
    icsum::BatchEngine eng(0);
    std::mt19937_64 rng(0x756e7772);
    auto bytes = [&](size_t n) {
        std::string s(n, '\0');
        for (auto& c : s) c = static_cast<char>(rng());
        return s;
    };
    auto message = [&](bool syn, bool rst, size_t payload) {
        TCPMessage m;
        m.sender.seqno = Wrap32{static_cast<uint32_t>(rng())};
        m.sender.SYN = syn;
        m.sender.RST = rst;
        m.sender.FIN = rng() % 7 == 0;
        m.sender.payload = bytes(payload);
        if (rng() % 3) m.receiver.ackno = Wrap32{static_cast<uint32_t>(rng())};
        m.receiver.window_size = static_cast<uint16_t>(rng());
        return m;
    };
    const Endpoints peer{"10.9.8.7", 80, "10.1.2.3", 4321};      // the peer of the adapters below
    const Endpoints stranger{"10.9.8.9", 80, "10.1.2.3", 4321};  // another host, same ports
    size_t total = 0;

    // a listening adapter that connects on the third datagram of the batch:
    // data without SYN, SYN + RST, the SYN; then the peer, a stranger, and the
    // peer again from another port
    {
        Run r;
        r.push(wire_of(peer, message(false, false, 100)));
        r.push(wire_of(peer, message(true, true, 0)));
        r.push(wire_of(peer, message(true, false, 0)));
        r.push(wire_of(peer, message(false, false, 333)));
        r.push(wire_of(stranger, message(false, false, 10)));
        r.push(wire_of(stranger, message(true, false, 0)));
        r.push(wire_of({"10.9.8.7", 81, "10.1.2.3", 4321}, message(false, false, 7)));
        r.push(wire_of(peer, message(false, false, 1000)));
        TCPOverIPv4Adapter L;
        L.config_mut().source = Address{"0", 4321};
        L.set_listening(true);
        const size_t acc = check_run(eng, r, L, false);
        EXPECT(acc == 3);  // the SYN and the peer's two data segments
        total += acc;
    }

    // a connected adapter with each gate wrong in turn
    {
        TCPOverIPv4Adapter C;
        C.config_mut().source = Address{"10.1.2.3", 4321};
        C.config_mut().destination = Address{"10.9.8.7", 80};
        Run r;
        r.push(wire_of(peer, message(false, false, 64)));                                     // passes
        r.push(wire_of({"10.9.8.8", 80, "10.1.2.3", 4321}, message(false, false, 64)));       // wrong src
        r.push(wire_of({"10.9.8.7", 80, "10.1.2.4", 4321}, message(false, false, 64)));       // wrong dst
        r.push(wire_of({"10.9.8.7", 81, "10.1.2.3", 4321}, message(false, false, 64)));       // wrong sport
        r.push(wire_of({"10.9.8.7", 80, "10.1.2.3", 4322}, message(false, false, 64)));       // wrong dport
        {  // wrong proto: 17, with the pseudo header's change taken out of the TCP checksum so both verify
            std::string w = wire_of(peer, message(false, false, 64));
            w[9] = 17;
            fix_ip(w);
            uint32_t ck = (static_cast<uint8_t>(w[36]) << 8) | static_cast<uint8_t>(w[37]);
            uint32_t s = (~ck & 0xffff) + 11;  // the sum the field complements grows by 17 - 6
            while (s > 0xffff) s = (s >> 16) + (s & 0xffff);
            put16(w, 36, ~s & 0xffff);
            r.push(w);
        }
        r.push(wire_of(peer, message(false, false, 1)));  // passes
        {  // corrupted payload, then a truncated datagram
            std::string w = wire_of(peer, message(false, false, 200));
            w[100] ^= 0x10;
            r.push(w);
            r.push(wire_of(peer, message(false, false, 200)).substr(0, 39));
        }
        const size_t acc = check_run(eng, r, C, false);
        EXPECT(acc == 2);
        total += acc;
        // the proto-17 datagram does verify: it is the gate that drops it
        const auto st = eng.verify_packed(reinterpret_cast<const uint8_t*>(r.arena.data()), r.off.data(), r.wires.size());
        EXPECT(st[5] == (ICS_ST_IPV4_OK | ICS_ST_TCP_CKSUM_OK | ICS_ST_TCP_HDR_OK));
    }

    // 6000 wires from the peer, strangers and wrong ports, a fifth corrupted,
    // some with IPv4 options in front of the TCP header, to a listening and to
    // a connected adapter
    {
        Run r;
        for (int i = 0; i < 6000; ++i) {
            const unsigned who = rng() % 8;
            const Endpoints e = who < 5    ? peer
                                : who == 5 ? stranger
                                : who == 6 ? Endpoints{"10.9.8.7", 81, "10.1.2.3", 4321}
                                           : Endpoints{"10.9.8.7", 80, "10.1.2.3", 4322};
            std::string w = wire_of(e, message(i == 1500 || rng() % 50 == 0, rng() % 40 == 0, rng() % 1001));
            if (rng() % 6 == 0) {  // 4 or 8 option bytes: hlen 6 / 7, len and checksum adjusted (options are not summed)
                const size_t opt = 4 * (1 + rng() % 2);
                w.insert(20, bytes(opt));
                w[0] = static_cast<char>(0x40 | (5 + opt / 4));
                put16(w, 2, static_cast<uint32_t>(w.size()));
                fix_ip(w);
            }
            if (rng() % 5 == 0) w[rng() % w.size()] ^= static_cast<char>(1u << (rng() % 8));
            r.push(w);
        }
        TCPOverIPv4Adapter L;
        L.config_mut().source = Address{"0", 4321};
        L.set_listening(true);
        TCPOverIPv4Adapter C;
        C.config_mut().source = Address{"10.1.2.3", 4321};
        C.config_mut().destination = Address{"10.9.8.7", 80};
        const size_t a1 = check_run(eng, r, L, false);
        const size_t a2 = check_run(eng, r, C, false);
        // listening: whoever sends the first clean SYN to port 4321 (the peer, 5/8 of the wires, or the
        // stranger, 1/8) is the only one accepted afterwards; connected: the peer's uncorrupted wires
        EXPECT(a1 > 300 && a2 > 2000);
        total += a1 + a2;
    }

    // an empty batch
    {
        TCPOverIPv4Adapter C;
        const uint64_t off0 = 0;
        EXPECT(eng.unwrap_records(C, nullptr, &off0, 0).empty());
    }

    std::printf("%s: unwrap_records == unwrap_packed == unwrap_tcp_in_ip (%zu accepted)\n", failures ? "FAILED" : "OK",
                total);
    return failures ? 1 : 0;
}
