// unwrap_loop.cpp — the host loop ics_tcp_unwrap_batch replaces, timed: one
// ics_tcp_unwrap_one per datagram (both checksums and the field parse, a
// 40-byte record out) over n datagrams with valid headers and checksums,
// split over `threads` threads.  Shapes: "mtu" = every datagram 1500 B, "mix" =
// half 40 B / half 1500 B.  Links icsum_unwrap.cpp alone:
//   g++ -O2 -std=c++17 -I include tools/probe/unwrap_loop.cpp
//       tcpip_network_protocol_stack_amd/csrc/icsum_unwrap.cpp -o tools/probe/unwrap_loop -lpthread
//   tools/probe/unwrap_loop <mtu|mix> <n> <threads>     -> one JSON line
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "icsum.h"

namespace {
uint32_t fold(uint32_t s) {
  while (s > 0xffffu) s = (s >> 16) + (s & 0xffffu);
  return ~s & 0xffffu;
}
void set16(uint8_t* p, uint32_t v) {
  p[0] = uint8_t(v >> 8);
  p[1] = uint8_t(v);
}
}  // namespace

int main(int argc, char** argv) {
  const std::string shape = argc > 1 ? argv[1] : "mtu";
  const size_t n = argc > 2 ? size_t(std::atoll(argv[2])) : size_t(1) << 20;
  const int threads = argc > 3 ? std::atoi(argv[3]) : 16;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&s] {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  };
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + (shape == "mix" && (rnd() >> 20) % 2 ? 40 : 1500);
  std::vector<uint8_t> buf(off[n] + 8);
  for (size_t k = 0; k + 8 <= buf.size(); k += 8) {
    const uint64_t v = rnd();
    std::memcpy(buf.data() + k, &v, 8);
  }
  for (size_t i = 0; i < n; ++i) {  // ver 4, hlen 5, len, DF, ttl 64, TCP, data offset 5, both checksums
    uint8_t* d = buf.data() + off[i];
    const uint32_t len = uint32_t(off[i + 1] - off[i]);
    d[0] = 0x45;
    d[1] = 0;
    set16(d + 2, len);
    set16(d + 6, 0x4000);
    d[8] = 64;
    d[9] = 6;
    d[32] = 0x50;
    set16(d + 36, 0);
    uint32_t t = 6 + (len - 20);
    for (int k = 12; k < 20; k += 2) t += (uint32_t(d[k]) << 8) | d[k + 1];
    for (uint32_t k = 20; k < len; ++k) t += (k & 1) ? d[k] : uint32_t(d[k]) << 8;
    set16(d + 36, fold(t));
    set16(d + 10, 0);
    uint32_t h = 0;
    for (int k = 0; k < 20; k += 2) h += (uint32_t(d[k]) << 8) | d[k + 1];
    set16(d + 10, fold(h));
  }
  std::vector<ics_tcp_rx> recs(n);
  std::vector<size_t> parsed(size_t(threads), 0);
  double best = 1e30;
  for (int rep = 0; rep < 3; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int w = 0; w < threads; ++w)
      th.emplace_back([&, w] {
        size_t p = 0;
        for (size_t i = n * size_t(w) / size_t(threads), e = n * size_t(w + 1) / size_t(threads); i < e; ++i) {
          ics_tcp_unwrap_one(buf.data() + off[i], size_t(off[i + 1] - off[i]), &recs[i]);
          p += size_t((recs[i].status & 7u) == 7u);
        }
        parsed[size_t(w)] = p;
      });
    for (auto& x : th) x.join();
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < best) best = us;
  }
  size_t p = 0;
  for (size_t x : parsed) p += x;
  std::printf("{\"row\": \"host_unwrap_loop\", \"shape\": \"%s\", \"n\": %zu, \"bytes\": %llu, \"threads\": %d, "
              "\"best_of_3_us\": %.1f, \"parsed\": %zu}\n",
              shape.c_str(), n, (unsigned long long)off[n], threads, best, p);
  return p == n ? 0 : 1;
}
