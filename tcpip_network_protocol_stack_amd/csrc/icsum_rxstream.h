// icsum_rxstream.h — the receive stream object behind ics_rx_stream_*
// (include/icsum.h): TCPReceiver + Reassembler + the writer half of ByteStream
// with lists of source ranges where the reference holds strings.  Shared by
// icsum_rxstream.cpp (plain C++, links alone: the control plane) and
// icsum_rxdev.cpp (the ring in device memory and the copy launch).  Not
// installed, not part of the ABI.
#pragma once

#include <cstdint>
#include <list>
#include <mutex>
#include <vector>

#include "icsum.h"

namespace icsum::rx {

// Where a run of an interval's bytes lives: in payload `rec` of the batch being
// planned, `off` bytes in — or already in the ring (kInRing), at its stream
// index mod capacity, which needs no offset.
constexpr uint32_t kInRing = 0xFFFFFFFFu;
struct Piece {
  uint32_t rec;
  uint32_t off;
  uint32_t len;
};

// Reassembler::Interval (reassembler.h:49-59) with `pieces` for interval_str:
// the pieces' lengths sum to end - beg.
struct Interval {
  uint64_t beg, end;
  std::vector<Piece> pieces;
};

// the reference's state, without the bytes
struct State {
  uint64_t capacity = 0;
  bool has_isn = false;
  uint32_t isn = 0;
  // bytes_pushed IS first_unassembled_index_: see push_ready (icsum_rxstream.cpp)
  uint64_t pushed = 0, popped = 0;
  uint64_t eof = UINT64_MAX;
  bool closed = false, error = false;
  std::list<Interval> bufs;
};

}  // namespace icsum::rx

struct ics_rx_stream {
  std::mutex mu;
  icsum::rx::State st;
  std::vector<ics_copy_piece> plan;  // the last batch's copy list (kept: it only grows)
  // the device half (icsum_rxdev.cpp); null for a host-only object
  ics_ctx* ctx = nullptr;
  void* d_ring = nullptr;
  void (*free_ring)(ics_rx_stream*) = nullptr;
};

namespace icsum::rx {

// ics_rx_stream_plan's body on state `s`: validates the batch (nothing is
// changed when that fails), runs receive over the taken records in order and
// leaves the batch's copy list in `out`.  The caller holds the stream's lock.
int run_plan(State& s, std::vector<ics_copy_piece>& out, const ics_tcp_rx* recs, uint64_t n, const uint8_t* take,
             const uint64_t* h_offsets, uint64_t stride, uint64_t dgram_len);

}  // namespace icsum::rx
