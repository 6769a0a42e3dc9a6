// icsum_rxstream.cpp — the receive stream's control plane (include/icsum.h,
// ics_rx_stream_*): TCPReceiver::receive (src/tcp_receiver/tcp_receiver.cpp:4-44),
// Wrap32::unwrap (src/wrapping_integers/wrapping_integers.cpp:18-31),
// Reassembler::insert (src/reassembler/reassembler.cpp:4-103) and the writer
// half of ByteStream (src/byte_stream/byte_stream.cpp:60-67), statement for
// statement and in the reference's order, with a list of source ranges
// (icsum::rx::Piece) wherever the reference holds a std::string.  No byte is
// touched here: a batch's plan ends in a copy list (ics_copy_piece) that
// k_copy_pieces, or a test's numpy ring, executes.  Plain C++: no HIP, no
// context, usable (and tested) on a machine without a GPU; it links alone.
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <new>

#include "icsum_rxstream.h"

namespace icsum::detail {
// icsum_api.cpp's error reporting; absent (null) when this file is linked alone
int fail(int code, const char* fmt, ...) __attribute__((weak, format(printf, 2, 3)));
}  // namespace icsum::detail

namespace icsum::rx {
namespace {

#define RX_FAIL(code, ...) (::icsum::detail::fail ? ::icsum::detail::fail((code), __VA_ARGS__) : (code))

static_assert(sizeof(ics_copy_piece) == 16 && offsetof(ics_copy_piece, dst) == 8 && offsetof(ics_copy_piece, len) == 12,
              "ics_copy_piece layout");

// Wrap32::unwrap with its conversions: the difference of the raw values as an
// int32_t, added to the uint64_t checkpoint (sign-extended), the sum read as an
// int64_t, 2^32 added when that is negative.
uint64_t unwrap32(uint32_t raw, uint32_t isn, uint64_t checkpoint) {
  const int32_t offset = int32_t(raw - (isn + uint32_t(checkpoint)));
  const int64_t absseq = int64_t(checkpoint + uint64_t(int64_t(offset)));
  return absseq < 0 ? uint64_t(absseq) + (uint64_t(1) << 32) : uint64_t(absseq);
}

uint64_t available(const State& s) { return s.capacity - (s.pushed - s.popped); }

// interval_str.substr(0, keep): the first `keep` bytes of a piece list
void keep_prefix(std::vector<Piece>& v, uint64_t keep) {
  size_t k = 0;
  for (; k < v.size() && keep >= v[k].len; ++k) keep -= v[k].len;
  if (k < v.size() && keep) {
    v[k].len = uint32_t(keep);
    ++k;
  }
  v.resize(k);
}

void append(std::vector<Piece>& v, const std::vector<Piece>& w) { v.insert(v.end(), w.begin(), w.end()); }

// The copy list of one batch, in increasing stream index.
struct Emit {
  std::vector<ics_copy_piece>& out;
  const ics_tcp_rx* recs;
  const uint64_t* offs;
  uint64_t stride;
  uint64_t capacity;
  // `len` bytes of record `rec`'s payload from `off` on are the stream's bytes
  // [idx, idx + len): split at the ring's wrap, joined to the piece before
  // when both sides continue it
  void bytes(uint64_t idx, uint32_t rec, uint32_t off, uint32_t len) {
    uint64_t src = (offs ? offs[rec] : uint64_t(rec) * stride) + recs[rec].pay_off + off;
    while (len) {
      const uint64_t dst = idx % capacity;
      const uint32_t run = uint32_t(std::min<uint64_t>(len, capacity - dst));
      if (!out.empty()) {
        ics_copy_piece& b = out.back();
        if (uint64_t(b.dst) + b.len == dst && b.src + b.len == src && uint64_t(b.len) + run <= 0xFFFFFFFFull) {
          b.len += run;
          src += run, idx += run, len -= run;
          continue;
        }
      }
      out.push_back(ics_copy_piece{src, uint32_t(dst), run});
      src += run, idx += run, len -= run;
    }
  }
  // every run of an interval that still lies in a record of this batch
  void interval(Interval& iv, bool to_ring) {
    uint64_t idx = iv.beg;
    for (Piece& p : iv.pieces) {
      if (p.rec != kInRing) bytes(idx, p.rec, p.off, p.len);
      idx += p.len;
    }
    if (to_ring) {  // the batch ends: its records go away, the bytes are in the ring
      uint64_t left = iv.end - iv.beg;
      iv.pieces.clear();
      for (; left; left -= std::min<uint64_t>(left, 0x80000000u))
        iv.pieces.push_back(Piece{kInRing, 0, uint32_t(std::min<uint64_t>(left, 0x80000000u))});
    }
  }
};

// The tail of Reassembler::insert (reassembler.cpp:86-102): intervals are
// pushed while their start equals first_unassembled_index_.
// bytes_pushed == first_unassembled_index_ at all times: an interval's end was
// clipped to first_unassembled_index_ + available_capacity() when it was
// inserted (reassembler.cpp:20-21), that sum is bytes_popped + capacity, which
// only grows, so Writer::push's min(data.size(), available_capacity())
// (byte_stream.cpp:64) never cuts what the Reassembler hands it, and both
// counters advance by the interval's whole length.  (insert returns at once on
// a closed writer, so push's other guards hold too.)
void push_ready(State& s, Emit& em) {
  for (auto it = s.bufs.begin(); it != s.bufs.end();) {
    if (it->beg == s.pushed) {
      em.interval(*it, false);
      s.pushed = it->end;
      it = s.bufs.erase(it);
    } else {
      ++it;
    }
  }
  if (s.pushed >= s.eof) s.closed = true;
}

// Reassembler::insert(first, payload of `len` bytes in record `rec`, last)
void insert(State& s, Emit& em, uint64_t first, uint32_t rec, uint32_t len, bool last) {
  const uint64_t edge = s.pushed + available(s);  // first_unassembled + available_capacity
  if (s.closed || first >= s.eof || first >= edge) return;
  if (last) s.eof = first + len;  // set even when the clipped range below is empty
  const uint64_t beg = std::max(first, s.pushed), end = std::min(first + len, edge);
  if (end <= beg) {
    if (s.pushed >= s.eof) s.closed = true;
    return;
  }
  Interval nv{beg, end, {Piece{rec, uint32_t(beg - first), uint32_t(end - beg)}}};
  if (s.bufs.empty()) {
    s.bufs.push_back(std::move(nv));
  } else {
    // std::lower_bound under Interval::operator< (reassembler.h:55-58): by beg, then end
    auto it = s.bufs.begin();
    while (it != s.bufs.end() && (it->beg != nv.beg ? it->beg < nv.beg : it->end < nv.end)) ++it;
    std::list<Interval>::iterator cur;  // the reference's `prev`; its copy `itv` is cur's beg / end
    if (it == s.bufs.begin()) {
      cur = s.bufs.insert(it, std::move(nv));
    } else {
      cur = std::prev(it);
      if (cur->end >= nv.beg) {      // touching intervals merge
        if (cur->end <= nv.end) {    // the new range wins its overlap with the one before
          keep_prefix(cur->pieces, nv.beg - cur->beg);
          append(cur->pieces, nv.pieces);
          cur->end = nv.end;
        }                            // else: wholly inside it, discarded
      } else {
        cur = s.bufs.insert(it, std::move(nv));
      }
    }
    while (it != s.bufs.end() && cur->end >= it->beg) {
      if (it->end > cur->end) {      // a following interval that ends later keeps its overlap
        keep_prefix(cur->pieces, it->beg - cur->beg);
        append(cur->pieces, it->pieces);
        cur->end = it->end;
      }                              // else: covered, erased
      it = s.bufs.erase(it);
    }
  }
  push_ready(s, em);
}

// TCPReceiver::receive of one record
void receive(State& s, Emit& em, const ics_tcp_rx& r, uint32_t rec) {
  if (s.error) return;
  if (r.msg.flags & ICS_TCP_RST) {
    s.error = true;
    return;
  }
  const bool syn = (r.msg.flags & ICS_TCP_SYN) != 0;
  if (!s.has_isn) {
    if (!syn) return;
    s.isn = r.msg.seqno;
    s.has_isn = true;
  }
  const uint64_t ckpt = s.pushed + 1;
  const uint64_t absseq = unwrap32(r.msg.seqno, s.isn, ckpt);
  const uint64_t idx = syn ? 0 : absseq - 1;  // absseq 0: UINT64_MAX, which `>= eof` rejects
  insert(s, em, idx, rec, r.pay_len, (r.msg.flags & ICS_TCP_FIN) != 0);
}

bool taken(const ics_tcp_rx& r, const uint8_t* take, uint64_t i) {
  return take ? take[i] != 0 : (r.status & 7u) == 7u && (r.status & ICS_ST_PROTO_TCP);
}

}  // namespace

int run_plan(State& s, std::vector<ics_copy_piece>& out, const ics_tcp_rx* recs, uint64_t n, const uint8_t* take,
             const uint64_t* h_offsets, uint64_t stride, uint64_t dgram_len) {
  out.clear();
  if (n && !recs) return RX_FAIL(ICS_ERR_INVALID, "null records");
  if (n >= kInRing) return RX_FAIL(ICS_ERR_INVALID, "%llu records in one batch (at most 2^32 - 2)", (unsigned long long)n);
  for (uint64_t i = 0; i < n; ++i) {
    if (h_offsets && h_offsets[i + 1] < h_offsets[i])
      return RX_FAIL(ICS_ERR_INVALID, "offsets decrease at datagram %llu", (unsigned long long)i);
    if (!taken(recs[i], take, i)) continue;
    const uint64_t len = h_offsets ? h_offsets[i + 1] - h_offsets[i] : dgram_len;
    if (uint64_t(recs[i].pay_off) + recs[i].pay_len > len)
      return RX_FAIL(ICS_ERR_INVALID, "record %llu: payload [%u, %u + %u) outside its datagram of %llu bytes",
                     (unsigned long long)i, recs[i].pay_off, recs[i].pay_off, recs[i].pay_len,
                     (unsigned long long)len);
  }
  try {
    Emit em{out, recs, h_offsets, stride, s.capacity};
    for (uint64_t i = 0; i < n; ++i)
      if (taken(recs[i], take, i)) receive(s, em, recs[i], uint32_t(i));
    for (Interval& iv : s.bufs) em.interval(iv, true);
  } catch (const std::bad_alloc&) {
    return RX_FAIL(ICS_ERR_NOMEM, "receive stream plan: out of host memory");
  }
  return ICS_OK;
}

}  // namespace icsum::rx

using icsum::rx::State;

extern "C" {

int ics_rx_stream_create_host(uint64_t capacity, ics_rx_stream** out) {
  if (!out) return RX_FAIL(ICS_ERR_INVALID, "null output pointer");
  *out = nullptr;
  if (capacity < 1 || capacity > (uint64_t(1) << 30))
    return RX_FAIL(ICS_ERR_INVALID, "stream capacity %llu outside 1 .. 2^30", (unsigned long long)capacity);
  ics_rx_stream* rxs = new (std::nothrow) ics_rx_stream();
  if (!rxs) return RX_FAIL(ICS_ERR_NOMEM, "stream allocation failed");
  rxs->st.capacity = capacity;
  *out = rxs;
  return ICS_OK;
}

int ics_rx_stream_destroy(ics_rx_stream* rxs) {
  if (!rxs) return ICS_OK;
  if (rxs->free_ring) rxs->free_ring(rxs);
  delete rxs;
  return ICS_OK;
}

int ics_rx_stream_plan(ics_rx_stream* rxs, const ics_tcp_rx* recs, uint64_t n, const uint8_t* take,
                       const uint64_t* h_offsets, uint64_t stride, uint64_t dgram_len, ics_copy_piece* pieces,
                       uint64_t cap, uint64_t* m) {
  if (!rxs) return RX_FAIL(ICS_ERR_INVALID, "null stream");
  if (!m) return RX_FAIL(ICS_ERR_INVALID, "null piece count");
  std::lock_guard<std::mutex> lock(rxs->mu);
  try {
    State w = rxs->st;  // the state changes only when the whole call succeeds
    if (int rc = icsum::rx::run_plan(w, rxs->plan, recs, n, take, h_offsets, stride, dgram_len)) return rc;
    const uint64_t count = rxs->plan.size();
    if (pieces) {
      if (count > cap)
        return RX_FAIL(ICS_ERR_INVALID, "piece array of %llu holds less than the plan's %llu pieces",
                       (unsigned long long)cap, (unsigned long long)count);
      std::copy(rxs->plan.begin(), rxs->plan.end(), pieces);
      rxs->st = std::move(w);
    }
    *m = count;
  } catch (const std::bad_alloc&) {
    return RX_FAIL(ICS_ERR_NOMEM, "receive stream plan: out of host memory");
  }
  return ICS_OK;
}

int ics_rx_stream_send(ics_rx_stream* rxs, ics_rx_send_t* out) {
  if (!rxs || !out) return RX_FAIL(ICS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(rxs->mu);
  const State& s = rxs->st;
  *out = ics_rx_send_t{};
  if (s.has_isn) {
    out->has_ackno = 1;
    out->ackno = s.isn + uint32_t(s.pushed + 1 + (s.closed ? 1 : 0));  // Wrap32::wrap
  }
  out->window = uint16_t(std::min<uint64_t>(icsum::rx::available(s), 65535));
  out->rst = s.error ? 1 : 0;
  return ICS_OK;
}

int ics_rx_stream_stats(ics_rx_stream* rxs, ics_rx_stats_t* out) {
  if (!rxs || !out) return RX_FAIL(ICS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(rxs->mu);
  const State& s = rxs->st;
  *out = ics_rx_stats_t{};
  out->capacity = s.capacity;
  out->bytes_pushed = s.pushed;
  out->bytes_popped = s.popped;
  out->bytes_buffered = s.pushed - s.popped;
  for (const auto& iv : s.bufs) out->bytes_pending += iv.end - iv.beg;
  out->available_capacity = icsum::rx::available(s);
  out->eof_index = s.eof;
  out->intervals = s.bufs.size();
  out->closed = s.closed;
  out->error = s.error;
  out->finished = s.closed && s.pushed == s.popped;
  out->has_isn = s.has_isn;
  return ICS_OK;
}

int ics_rx_stream_pop(ics_rx_stream* rxs, uint64_t len) {
  if (!rxs) return RX_FAIL(ICS_ERR_INVALID, "null stream");
  std::lock_guard<std::mutex> lock(rxs->mu);
  State& s = rxs->st;
  if (len > s.pushed - s.popped)
    return RX_FAIL(ICS_ERR_INVALID, "pop of %llu bytes with %llu buffered", (unsigned long long)len,
                   (unsigned long long)(s.pushed - s.popped));
  s.popped += len;
  return ICS_OK;
}

int ics_rx_stream_peek(ics_rx_stream* rxs, uint32_t off[2], uint32_t len[2], uint32_t* ranges) {
  if (!rxs || !off || !len || !ranges) return RX_FAIL(ICS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lock(rxs->mu);
  const State& s = rxs->st;
  const uint64_t have = s.pushed - s.popped, at = s.popped % s.capacity;
  const uint64_t first = std::min(have, s.capacity - at);
  off[0] = uint32_t(at), len[0] = uint32_t(first);
  off[1] = 0, len[1] = uint32_t(have - first);
  *ranges = have == 0 ? 0u : (len[1] ? 2u : 1u);
  return ICS_OK;
}

int ics_rx_stream_set_error(ics_rx_stream* rxs) {
  if (!rxs) return RX_FAIL(ICS_ERR_INVALID, "null stream");
  std::lock_guard<std::mutex> lock(rxs->mu);
  rxs->st.error = true;
  return ICS_OK;
}

}  // extern "C"
