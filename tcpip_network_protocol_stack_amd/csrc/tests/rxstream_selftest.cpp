// rxstream_selftest.cpp — icsum_rxstream.cpp linked alone (no HIP, no
// context), built with ASan + UBSan by tests/test_rx_stream.py and run as a
// child process.
//   1. The merge branches of include/icsum.h by hand, conflicting bytes, the
//      popped stream compared with what the rules say.
//   2. 100 000 random inserts at capacity 64 (1..4 records per plan, random
//      bytes, so every overlap conflicts; pops in between; a FIN near the end)
//      against a byte-array model: the model keeps `have` / `val` per stream
//      index and decides each new range byte-wise from the maximal runs
//      around it — written from the rules, not from the interval list.  After
//      every plan the pieces are applied to a 64-byte ring and every held
//      byte, pending or buffered, is compared.
//   3. Every plan's piece array is a heap block of exactly m pieces (a write
//      behind it trips the sanitizer), and one piece less is refused with the
//      state unchanged.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
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

uint32_t g_state = 0x5eed;
uint32_t rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state >> 8;
}

char g_summary[160];
constexpr uint32_t kIsn = 0xFFFFFF80u;  // the stream crosses 2^32 in sequence space
constexpr uint32_t kHdr = 40;

struct Seg {
  int64_t idx;  // stream index of the first payload byte (SYN: ignored)
  std::vector<uint8_t> bytes;
  bool syn = false, fin = false;
};

// a batch as the library takes it: records, offsets, and the datagram buffer
struct Batch {
  std::vector<ics_tcp_rx> recs;
  std::vector<uint64_t> off;
  std::vector<uint8_t> buf;
  explicit Batch(const std::vector<Seg>& segs) {
    off.push_back(0);
    for (const Seg& s : segs) {
      ics_tcp_rx r{};
      r.msg.seqno = s.syn ? kIsn : kIsn + 1u + uint32_t(s.idx);
      r.msg.flags = uint8_t((s.syn ? ICS_TCP_SYN : 0) | (s.fin ? ICS_TCP_FIN : 0));
      r.pay_off = kHdr;
      r.pay_len = uint32_t(s.bytes.size());
      r.status = ICS_ST_ACCEPT;
      recs.push_back(r);
      buf.insert(buf.end(), kHdr, 0xEE);
      buf.insert(buf.end(), s.bytes.begin(), s.bytes.end());
      off.push_back(buf.size());
    }
  }
};

// the byte-array model
struct Model {
  uint64_t cap;
  uint64_t pushed = 0, popped = 0, eof = UINT64_MAX;
  bool closed = false;
  std::vector<uint8_t> have, val;
  explicit Model(uint64_t c, size_t room) : cap(c), have(room, 0), val(room, 0) {}
  uint64_t run_end(uint64_t i) const {  // end of the maximal run holding byte i
    while (have[i]) ++i;
    return i;
  }
  void insert(int64_t first_signed, const std::vector<uint8_t>& b, bool fin) {
    if (first_signed < 0) return;  // absseq 0 or "negative": rejected far beyond the window
    const uint64_t first = uint64_t(first_signed), edge = popped + cap;
    if (closed || first >= eof || first >= edge) return;
    if (fin) eof = first + b.size();
    const uint64_t beg = first > pushed ? first : pushed;
    const uint64_t end = first + b.size() < edge ? first + b.size() : edge;
    if (end > beg) {
      bool write = true;
      if (have[beg]) {
        // The run holding the first byte.  Starting before it (or with it and ending first), it is the
        // interval before the new range: reaching past the new range's end it holds it whole and the new
        // range is discarded, else the new range wins.  Starting with it and ending behind it, it keeps all
        // of it.  Either way: nothing is written when the run ends later, and the new range wins when not.
        if (run_end(beg) > end) write = false;
      }
      if (write) {
        // up to the start of the first following run that ends later (it keeps its overlap);
        // runs that end inside the new range are covered
        uint64_t stop = end;
        for (uint64_t i = beg + 1; i < end; ++i)
          if (have[i] && !have[i - 1] && run_end(i) > end) {
            stop = i;
            break;
          }
        for (uint64_t i = beg; i < stop; ++i) have[i] = 1, val[i] = b[i - first];
      }
      while (have[pushed]) ++pushed;  // (the hole at `pushed` filled: the run is pushed)
    }
    if (pushed >= eof) closed = true;
  }
  uint64_t pending() const {
    uint64_t n = 0;
    for (uint64_t i = pushed; i < popped + cap; ++i) n += have[i];
    return n;
  }
};

struct Stream {
  ics_rx_stream* rxs = nullptr;
  std::vector<uint8_t> ring;
  explicit Stream(uint64_t cap) : ring(cap, 0x5A) { EXPECT(ics_rx_stream_create_host(cap, &rxs) == ICS_OK); }
  ~Stream() { ics_rx_stream_destroy(rxs); }
  // plan with a piece array of exactly the plan's size, pieces applied to the ring
  void plan(const Batch& b, bool try_short) {
    uint64_t m = 0, m2 = 99;
    EXPECT(ics_rx_stream_plan(rxs, b.recs.data(), b.recs.size(), nullptr, b.off.data(), 0, 0, nullptr, 0, &m) == ICS_OK);
    ics_rx_stats_t before{}, after{};
    ics_rx_stream_stats(rxs, &before);
    if (try_short && m > 0) {
      std::unique_ptr<ics_copy_piece[]> few(new ics_copy_piece[m - 1]);
      EXPECT(ics_rx_stream_plan(rxs, b.recs.data(), b.recs.size(), nullptr, b.off.data(), 0, 0, few.get(), m - 1, &m2) ==
             ICS_ERR_INVALID);
      ics_rx_stream_stats(rxs, &after);
      EXPECT(m2 == 99 && std::memcmp(&before, &after, sizeof before) == 0);
    }
    std::unique_ptr<ics_copy_piece[]> pieces(new ics_copy_piece[m]);
    EXPECT(ics_rx_stream_plan(rxs, b.recs.data(), b.recs.size(), nullptr, b.off.data(), 0, 0, pieces.get(), m, &m2) ==
           ICS_OK);
    EXPECT(m2 == m);
    for (uint64_t k = 0; k < m; ++k) {
      const ics_copy_piece& p = pieces[k];
      EXPECT(p.len > 0 && uint64_t(p.dst) + p.len <= ring.size() && p.src + p.len <= b.buf.size());
      if (uint64_t(p.dst) + p.len <= ring.size() && p.src + p.len <= b.buf.size())
        std::memcpy(ring.data() + p.dst, b.buf.data() + p.src, p.len);
    }
  }
  std::vector<uint8_t> pop(uint64_t n) {
    uint32_t off[2], len[2], k = 0;
    EXPECT(ics_rx_stream_peek(rxs, off, len, &k) == ICS_OK);
    std::vector<uint8_t> out;
    for (uint32_t i = 0; i < k; ++i) out.insert(out.end(), ring.begin() + off[i], ring.begin() + off[i] + len[i]);
    if (out.size() > n) out.resize(n);
    EXPECT(ics_rx_stream_pop(rxs, out.size()) == ICS_OK);
    return out;
  }
};

std::vector<uint8_t> fill(size_t n, uint8_t v) { return std::vector<uint8_t>(n, v); }

// pending ranges (index, length, fill byte) behind a hole at [0, 4), the hole
// filled with '.', everything popped: the stream as a string
std::string merged(const std::vector<Seg>& segs) {
  Stream s(64);
  std::vector<Seg> all{Seg{0, {}, true, false}};
  all.insert(all.end(), segs.begin(), segs.end());
  all.push_back(Seg{0, fill(4, '.'), false, false});
  for (const Seg& g : all) s.plan(Batch({g}), true);  // one record per plan
  const std::vector<uint8_t> a = s.pop(64);
  Stream t(64);
  t.plan(Batch(all), true);  // ... and all in one
  const std::vector<uint8_t> b = t.pop(64);
  EXPECT(a == b);
  return std::string(a.begin(), a.end());
}

void merge_branches() {
  auto S = [](int64_t idx, size_t n, char c) { return Seg{idx, fill(n, uint8_t(c)), false, false}; };
  EXPECT(merged({S(4, 4, 'a'), S(8, 4, 'b')}) == "....aaaabbbb");                    // touching intervals merge
  EXPECT(merged({S(4, 10, 'a'), S(6, 3, 'b')}) == "....aaaaaaaaaa");                 // wholly inside: discarded
  EXPECT(merged({S(4, 10, 'a'), S(6, 8, 'b')}) == "....aabbbbbbbb");                 // same end: the new range wins
  EXPECT(merged({S(4, 6, 'a'), S(7, 6, 'b')}) == "....aaabbbbbb");                   // wins its overlap with prev
  EXPECT(merged({S(4, 4, 'a'), S(4, 9, 'b')}) == "....bbbbbbbbb");                   // same start, longer: wins all
  EXPECT(merged({S(4, 9, 'a'), S(4, 4, 'b')}) == "....aaaaaaaaa");                   // same start, shorter: old keeps
  EXPECT(merged({S(4, 6, 'a'), S(4, 6, 'b')}) == "....bbbbbb");                      // a duplicate: erased, new wins
  EXPECT(merged({S(8, 6, 'a'), S(4, 7, 'b')}) == "....bbbbaaaaaa");                  // a following one ending later keeps
  EXPECT(merged({S(8, 3, 'a'), S(4, 10, 'b')}) == "....bbbbbbbbbb");                 // a covered one is erased
  EXPECT(merged({S(8, 4, 'a'), S(4, 8, 'b')}) == "....bbbbbbbb");                    // same end behind: erased
  EXPECT(merged({S(4, 4, 'a'), S(12, 4, 'b'), S(20, 6, 'c'), S(6, 16, 'd')}) == "....aaddddddddddddddcccccc");
  EXPECT(merged({S(6, 2, 'a'), S(10, 2, 'b'), S(14, 2, 'c'), S(4, 20, 'd')}) == "....dddddddddddddddddddd");
  EXPECT(merged({S(4, 6, 'a'), S(14, 6, 'b'), S(8, 8, 'c')}) == "....aaaaccccccbbbbbb");
}

void random_inserts() {
  constexpr uint64_t kCap = 64;
  constexpr int kInserts = 100000;
  Model model(kCap, size_t(kInserts) * 26 + 4096);
  Stream s(kCap);
  s.plan(Batch({Seg{0, {}, true, false}}), false);
  int done = 0, plans = 0;
  uint64_t popped_total = 0;
  while (done < kInserts) {
    std::vector<Seg> segs;
    const int k = 1 + int(rnd() % 4);
    for (int j = 0; j < k; ++j, ++done) {
      Seg g;
      const uint32_t len = rnd() % 25;
      const uint32_t u = rnd() % 10;
      if (u < 3)
        g.idx = int64_t(model.pushed) - int64_t(rnd() % 4);
      else
        g.idx = int64_t(model.pushed) - 20 + int64_t(rnd() % (kCap + 45));
      for (uint32_t b = 0; b < len; ++b) g.bytes.push_back(uint8_t(rnd()));
      g.fin = done > kInserts - 40 && rnd() % 8 == 0;
      segs.push_back(g);
    }
    const Batch b(segs);
    s.plan(b, ++plans % 7 == 0);
    // the model takes the same segments one by one; its window does not move inside a batch
    for (const Seg& g : segs) model.insert(g.idx, g.bytes, g.fin);
    ics_rx_stats_t st{};
    EXPECT(ics_rx_stream_stats(s.rxs, &st) == ICS_OK);
    EXPECT(st.bytes_pushed == model.pushed && st.bytes_popped == model.popped && st.bytes_pending == model.pending());
    EXPECT((st.closed != 0) == model.closed && st.eof_index == model.eof);
    for (uint64_t i = model.popped; i < model.popped + kCap; ++i)
      if (i < model.pushed || model.have[i]) EXPECT(s.ring[i % kCap] == model.val[i]);
    if (failures) break;
    if (rnd() % 3 == 0) {
      const uint64_t n = rnd() % 40;
      const std::vector<uint8_t> got = s.pop(n);
      const uint64_t want = n < model.pushed - model.popped ? n : model.pushed - model.popped;
      EXPECT(got.size() == want);
      for (uint64_t i = 0; i < got.size() && i < want; ++i) EXPECT(got[i] == model.val[model.popped + i]);
      model.popped += want;
      popped_total += want;
    }
  }
  EXPECT(popped_total > 50000);  // the ring wrapped many hundred times
  ics_rx_send_t snd{};
  EXPECT(ics_rx_stream_send(s.rxs, &snd) == ICS_OK);
  EXPECT(snd.has_ackno && snd.ackno == kIsn + uint32_t(model.pushed + 1 + (model.closed ? 1 : 0)));
  std::snprintf(g_summary, sizeof g_summary, "random inserts: %d in %d plans, %llu bytes popped, closed %d", done, plans,
                (unsigned long long)popped_total, int(model.closed));
}

}  // namespace

int main() {
  merge_branches();
  random_inserts();
  if (failures) {
    std::printf("rxstream_selftest FAILED: %d\n", failures);
    return 1;
  }
  std::printf("rxstream_selftest ok\n%s\n", g_summary);
  return 0;
}
