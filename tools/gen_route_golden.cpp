// gen_route_golden.cpp — writes tests/golden/route_cases.json from the real
// reference's Router::add_route / Router::match (src/router/router.cpp).
// Run once by hand where the reference tree is checked out; not part of
// build(), and nothing at test time needs it.  It includes the reference's
// headers and links its sources; it contains none of its text.
//
//   REF=<the reference tree>
//   g++ -std=gnu++20 -O1 -w $(for d in $REF/util/*/ $REF/src/*/; do echo -I$d; done)
//       tools/gen_route_golden.cpp $REF/src/router/router.cpp
//       $REF/src/network_interface/network_interface.cpp $REF/util/address/address.cpp
//       $REF/util/ipv4_header/ipv4_header.cpp $REF/util/ethernet/ethernet_header.cpp
//       $REF/util/arp_message/arp_message.cpp -o gen_route_golden
//   ./gen_route_golden > tests/golden/route_cases.json 2> /dev/null   # add_route logs to stderr
//
// Output: {"tables": [{"name", "routes": [[prefix, len, iface, has_next_hop,
// next_hop], ...] in add order, "addrs": [...], "answers": [[matched, iface,
// has_next_hop, next_hop], ...]}]} — all numbers host-order integers.
#include <array>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <optional>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

// Router::match is private; the generator is the one place that may ask
#define private public
#include "router.h"
#undef private

namespace {

struct R {
  uint32_t prefix, len, iface;
  bool has_nh;
  uint32_t nh;
};

uint64_t g_s = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_s ^= g_s << 13;
  g_s ^= g_s >> 7;
  g_s ^= g_s << 17;
  return uint32_t(g_s >> 16);
}

uint32_t mask_of(uint32_t len) { return len == 0 ? 0u : ~uint32_t(0) << (32 - len); }

bool g_first = true;

void emit(const std::string& name, const std::vector<R>& routes, std::vector<uint32_t> addrs, int extra_random) {
  Router router;
  for (const R& r : routes)
    router.add_route(r.prefix, uint8_t(r.len),
                     r.has_nh ? std::optional<Address>(Address::from_ipv4_numeric(r.nh)) : std::nullopt, r.iface);
  for (const R& r : routes) {
    // the range the route would cover were its host bits clear, and its neighbours
    const uint32_t m = mask_of(r.len), first = r.prefix & m, last = first | ~m;
    for (uint32_t a : {first, last, first - 1u, last + 1u, r.prefix}) {
      addrs.push_back(a);
      addrs.push_back(a ^ 1u);
    }
  }
  for (int k = 0; k < extra_random; ++k) addrs.push_back(rnd());
  std::printf("%s\n{\"name\": \"%s\", \"routes\": [", g_first ? "" : ",", name.c_str());
  g_first = false;
  for (size_t k = 0; k < routes.size(); ++k)
    std::printf("%s[%u, %u, %u, %d, %u]", k ? ", " : "", routes[k].prefix, routes[k].len, routes[k].iface,
                int(routes[k].has_nh), routes[k].nh);
  std::printf("],\n \"addrs\": [");
  for (size_t k = 0; k < addrs.size(); ++k) std::printf("%s%u", k ? ", " : "", addrs[k]);
  std::printf("],\n \"answers\": [");
  for (size_t k = 0; k < addrs.size(); ++k) {
    const auto hit = router.match(addrs[k]);
    if (!hit) {
      std::printf("%s[0, 0, 0, 0]", k ? ", " : "");
    } else {
      const bool has = hit->second.has_value();
      std::printf("%s[1, %zu, %d, %u]", k ? ", " : "", hit->first, int(has), has ? hit->second->ipv4_numeric() : 0u);
    }
  }
  std::printf("]}");
}

uint32_t ip(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a << 24 | b << 16 | c << 8 | d; }

}  // namespace

int main() {
  std::printf("{\"tables\": [");
  const std::vector<uint32_t> probes = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0xfffffffeu, ip(10, 0, 0, 1)};
  emit("empty", {}, probes, 20);
  emit("default_alone", {{0, 0, 1, false, 0}}, probes, 20);
  emit("default_with_next_hop", {{0, 0, 2, true, ip(192, 168, 0, 1)}}, probes, 20);
  emit("default_nonzero_prefix_is_dead", {{ip(10, 0, 0, 0), 0, 3, false, 0}, {1, 0, 4, false, 0}}, probes, 20);
  emit("dead_default_beside_live", {{ip(10, 0, 0, 0), 0, 3, false, 0}, {ip(10, 0, 0, 0), 8, 5, false, 0}}, probes, 20);
  emit("nested_15_16_17",
       {{ip(10, 2, 0, 0), 15, 1, false, 0}, {ip(10, 2, 0, 0), 16, 2, true, ip(1, 1, 1, 1)},
        {ip(10, 2, 128, 0), 17, 3, false, 0}, {ip(10, 3, 0, 0), 17, 4, true, ip(2, 2, 2, 2)}},
       probes, 30);
  emit("nested_23_24_25",
       {{ip(172, 16, 4, 0), 23, 1, false, 0}, {ip(172, 16, 4, 0), 24, 2, true, ip(3, 3, 3, 3)},
        {ip(172, 16, 4, 128), 25, 3, false, 0}, {ip(172, 16, 5, 0), 25, 4, false, 0},
        {ip(172, 16, 0, 0), 12, 5, false, 0}},
       probes, 30);
  emit("nested_30_31",
       {{ip(192, 168, 1, 4), 30, 1, false, 0}, {ip(192, 168, 1, 4), 31, 2, false, 0},
        {ip(192, 168, 1, 6), 31, 3, true, ip(4, 4, 4, 4)}, {ip(192, 168, 1, 0), 24, 4, false, 0},
        {ip(192, 168, 1, 254), 31, 5, false, 0}},
       probes, 30);
  emit("all_levels_nested",
       {{0, 0, 9, true, ip(9, 9, 9, 9)}, {ip(10, 0, 0, 0), 8, 1, false, 0}, {ip(10, 1, 0, 0), 16, 2, false, 0},
        {ip(10, 1, 2, 0), 24, 3, false, 0}, {ip(10, 1, 2, 64), 26, 4, false, 0}, {ip(10, 1, 2, 66), 31, 5, false, 0},
        {ip(10, 1, 2, 0), 20, 6, false, 0}, {ip(128, 0, 0, 0), 1, 7, false, 0}},
       probes, 40);
  emit("duplicates_overwrite",
       {{ip(10, 0, 0, 0), 8, 1, false, 0}, {ip(10, 0, 0, 0), 8, 2, true, ip(5, 5, 5, 5)},
        {ip(10, 9, 0, 0), 16, 3, true, ip(6, 6, 6, 6)}, {ip(10, 9, 0, 0), 16, 4, false, 0},
        {ip(10, 9, 9, 0), 25, 5, false, 0}, {ip(10, 9, 9, 0), 25, 6, false, 0}, {ip(10, 9, 9, 0), 25, 7, false, 0},
        {0, 0, 8, false, 0}, {0, 0, 9, false, 0}},
       probes, 30);
  emit("next_hop_zero_is_not_direct",
       {{ip(10, 0, 0, 0), 8, 1, true, 0}, {ip(10, 1, 0, 0), 17, 2, true, 0}, {ip(10, 1, 1, 0), 27, 3, true, 0},
        {ip(11, 0, 0, 0), 8, 4, false, 0}},
       probes, 30);
  emit("host_bits_set_are_dead",
       {{ip(10, 0, 0, 1), 8, 1, false, 0}, {ip(10, 0, 0, 0), 8, 2, false, 0}, {ip(10, 1, 128, 0), 16, 3, false, 0},
        {ip(10, 1, 0, 0), 16, 4, false, 0}, {ip(10, 1, 2, 3), 24, 5, false, 0}, {ip(10, 1, 2, 3), 31, 6, false, 0},
        {ip(10, 1, 2, 2), 31, 7, false, 0}, {ip(10, 1, 2, 129), 25, 8, false, 0}, {0x80000000u, 0, 9, false, 0},
        {ip(12, 0, 0, 0), 7, 10, false, 0}, {ip(13, 0, 0, 0), 7, 11, false, 0}},
       probes, 30);
  emit("large_iface_numbers", {{ip(10, 0, 0, 0), 8, 0x7fffffffu, false, 0}, {ip(10, 128, 0, 0), 9, 0, true, 0xffffffffu}},
       probes, 10);
  // random tables: prefixes drawn from a few bases so they nest, some dead, some duplicated
  for (int t = 0; t < 6; ++t) {
    std::vector<R> routes;
    const uint32_t bases[4] = {rnd(), rnd(), ip(10, 0, 0, 0) | (rnd() & 0xffff), rnd()};
    const int n = 20 + int(rnd() % 80);
    for (int k = 0; k < n; ++k) {
      uint32_t len = t % 2 ? 2 + rnd() % 30 : rnd() % 32;  // odd tables: no default route, so some addresses miss
      const uint32_t base = bases[rnd() % 4] ^ (rnd() % 4 == 0 ? rnd() & 0xffffu : 0u);
      uint32_t prefix = base & mask_of(len);
      if (rnd() % 7 == 0) prefix |= 1u << (rnd() % (32 - len));  // a host bit: dead
      if (rnd() % 6 == 0 && !routes.empty()) {                   // a duplicate key: overwrite
        const R& o = routes[rnd() % routes.size()];
        prefix = o.prefix;
        len = o.len;
      }
      const bool has = rnd() % 2;
      routes.push_back({prefix, len, rnd() % 16, has, has ? (rnd() % 5 == 0 ? 0u : rnd()) : 0u});
    }
    emit("random_" + std::to_string(t), routes, probes, 100);
  }
  std::printf("\n]}\n");
  return 0;
}
