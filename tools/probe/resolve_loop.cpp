// resolve_loop.cpp — the host loop ics_router_frames replaces, timed: one
// ics_neigh_table_resolve per datagram (a hash lookup and a 14-byte header
// build under the table's mutex) over n (interface, next hop) pairs, 9 in 10
// of them known, split over `threads` threads.  Links icsum_neigh.cpp alone:
//   g++ -O2 -std=c++17 -I include -I tcpip_network_protocol_stack_amd/csrc tools/probe/resolve_loop.cpp
//       tcpip_network_protocol_stack_amd/csrc/icsum_neigh.cpp -o tools/probe/resolve_loop -lpthread
//   tools/probe/resolve_loop <mappings> <n> <threads>     -> one JSON line
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "icsum.h"

int main(int argc, char** argv) {
  const uint32_t mappings = argc > 1 ? uint32_t(std::atoi(argv[1])) : 1000;
  const size_t n = argc > 2 ? size_t(std::atoll(argv[2])) : size_t(1) << 20;
  const int threads = argc > 3 ? std::atoi(argv[3]) : 16;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&s] {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return uint32_t(s >> 16);
  };
  ics_neigh_table* t = nullptr;
  if (ics_neigh_table_create(&t) != ICS_OK) return 1;
  for (uint32_t f = 0; f < 8; ++f) {
    const uint8_t mac[6] = {2, 0, 0, 0, 0, uint8_t(f)};
    ics_neigh_table_set_iface(t, f, mac, 0x0A000001u + (f << 8));
  }
  std::vector<uint32_t> ips(mappings);
  for (uint32_t k = 0; k < mappings; ++k) {
    ips[k] = rnd();
    const uint8_t mac[6] = {6, uint8_t(k >> 24), uint8_t(k >> 16), uint8_t(k >> 8), uint8_t(k), 1};
    ics_neigh_table_learn(t, k % 8, ips[k], mac);
  }
  std::vector<uint32_t> q_if(n), q_ip(n);
  for (size_t i = 0; i < n; ++i) {
    const uint32_t k = rnd() % (mappings ? mappings : 1);
    const bool known = mappings && rnd() % 10 != 0;
    q_if[i] = k % 8;
    q_ip[i] = known ? ips[k] : rnd();
  }
  std::vector<uint8_t> hdrs(14 * n);
  std::vector<size_t> hits(size_t(threads), 0);
  double best = 1e30;
  for (int rep = 0; rep < 5; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int w = 0; w < threads; ++w)
      th.emplace_back([&, w] {
        uint8_t req[42];
        uint32_t ev;
        size_t h = 0;
        for (size_t i = n * size_t(w) / size_t(threads), e = n * size_t(w + 1) / size_t(threads); i < e; ++i)
          h += size_t(ics_neigh_table_resolve(t, q_if[i], q_ip[i], hdrs.data() + 14 * i, &ev, req) == 1);
        hits[size_t(w)] = h;
      });
    for (auto& x : th) x.join();
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < best) best = us;
  }
  size_t h = 0;
  for (size_t x : hits) h += x;
  std::printf("{\"row\": \"host_resolve_loop\", \"mappings\": %u, \"n\": %zu, \"threads\": %d, \"best_of_5_us\": %.1f, "
              "\"resolved\": %zu}\n", mappings, n, threads, best, h);
  ics_neigh_table_destroy(t);
  return 0;
}
