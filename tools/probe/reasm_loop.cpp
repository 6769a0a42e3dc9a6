// reasm_loop.cpp — the host payload path ics_rx_stream_receive_batch replaces,
// timed: per accepted datagram the one payload copy BatchEngine::unwrap_records
// makes into a std::string, then the string operations the reference's receive
// path performs on it for an in-order segment, in the reference's shape —
// Reassembler::insert's data.substr into the interval (reassembler.cpp:34), the
// interval copied into the list (:39), Writer::push taking its string by value
// (:91) and push's data.substr into the deque (byte_stream.cpp:65) — and a
// reader that pops whole strings once a MiB is buffered.  The records (where
// each payload lies) are given: their parse is the device's either way.  Every
// thread runs its own connection over a contiguous share of the datagrams.
// Shapes: "mtu" = 1460 B payloads in 1500 B datagrams, "small" = 100 B in
// 140 B, "tick" = half 40 B ACKs (no payload) / half 1500 B.  Rounds alternate
// between the thread counts given.  No library needed:
//   g++ -O2 -std=c++17 tools/probe/reasm_loop.cpp -o tools/probe/reasm_loop -lpthread
//   tools/probe/reasm_loop <mtu|small|tick> <n> <threads,threads,...> <rounds>  -> one JSON line per thread count
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <list>
#include <string>
#include <thread>
#include <vector>

namespace {

struct Interval {
  uint64_t beg, end;
  std::string str;
};

// one connection's share: datagrams [i0, i1); returns the bytes pushed
uint64_t run(const uint8_t* arena, const uint64_t* off, const uint32_t* pay_len, size_t i0, size_t i1) {
  std::list<Interval> pending;
  std::deque<std::string> stream;
  uint64_t first_unassembled = 0, buffered = 0;
  for (size_t i = i0; i < i1; ++i) {
    if (!pay_len[i]) continue;
    std::string payload(reinterpret_cast<const char*>(arena) + off[i] + 40, pay_len[i]);  // unwrap_records
    Interval itv{first_unassembled, first_unassembled + payload.size(), payload.substr(0, payload.size())};
    pending.push_back(itv);
    for (auto it = pending.begin(); it != pending.end();) {
      if (it->beg == first_unassembled) {
        std::string data = it->str;  // push(std::string data)
        stream.emplace_back(data.substr(0, data.size()));
        buffered += data.size();
        first_unassembled = it->end;
        it = pending.erase(it);
      } else {
        ++it;
      }
    }
    if (buffered > (1u << 20)) {  // the reader
      stream.clear();
      buffered = 0;
    }
  }
  return first_unassembled;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string shape = argc > 1 ? argv[1] : "mtu";
  const size_t n = argc > 2 ? size_t(std::atoll(argv[2])) : size_t(1) << 20;
  std::vector<int> counts;
  for (const char* p = argc > 3 ? argv[3] : "1,16"; *p;) {
    counts.push_back(std::atoi(p));
    while (*p && *p != ',') ++p;
    if (*p) ++p;
  }
  const int rounds = argc > 4 ? std::atoi(argv[4]) : 9;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&s] {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  };
  std::vector<uint64_t> off(n + 1, 0);
  std::vector<uint32_t> pay(n);
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t len = shape == "mtu" ? 1500u : shape == "small" ? 140u : (rnd() & 1) ? 1500u : 40u;
    pay[i] = len - 40;
    off[i + 1] = off[i] + len;
    total += pay[i];
  }
  std::vector<uint8_t> arena(off[n]);
  for (size_t k = 0; k < arena.size(); k += 8) {
    const uint64_t v = rnd();
    std::memcpy(arena.data() + k, &v, std::min<size_t>(8, arena.size() - k));
  }
  std::vector<std::vector<double>> us(counts.size());
  for (int r = 0; r < rounds + 1; ++r) {
    for (size_t c = 0; c < counts.size(); ++c) {
      const int T = counts[c];
      std::vector<uint64_t> pushed(T, 0);
      const auto t0 = std::chrono::steady_clock::now();
      std::vector<std::thread> th;
      for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] { pushed[t] = run(arena.data(), off.data(), pay.data(), n * t / T, n * (t + 1) / T); });
      for (auto& x : th) x.join();
      const double d = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      uint64_t sum = 0;
      for (uint64_t v : pushed) sum += v;
      if (sum != total) {
        std::fprintf(stderr, "pushed %llu of %llu\n", (unsigned long long)sum, (unsigned long long)total);
        return 1;
      }
      if (r) us[c].push_back(d);  // round 0 warms up
    }
  }
  for (size_t c = 0; c < counts.size(); ++c) {
    std::sort(us[c].begin(), us[c].end());
    const auto& x = us[c];
    std::printf("{\"shape\": \"%s\", \"row\": \"host_path\", \"threads\": %d, \"n\": %zu, \"bytes\": %llu, "
                "\"median_us\": %.1f, \"p10_us\": %.1f, \"p90_us\": %.1f, \"rounds\": %zu}\n",
                shape.c_str(), counts[c], n, (unsigned long long)total, x[x.size() / 2], x[x.size() / 10],
                x[(9 * x.size()) / 10], x.size());
  }
  return 0;
}
