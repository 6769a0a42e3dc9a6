// icsum_rxdev.cpp — the device half of the receive streams (include/icsum.h):
// the ring in device memory, ics_rx_stream_receive_batch (plan on the host,
// icsum_rxstream.cpp; the copy list through ics_ctx::rx_pieces to the device;
// k_copy_pieces on the caller's stream) and ics_rx_stream_read.
#include <algorithm>
#include <cstring>
#include <new>

#include "icsum_ctx.h"
#include "icsum_rxstream.h"

using namespace icsum::detail;

namespace {

void free_ring(ics_rx_stream* rxs) {
  if (rxs->d_ring && rxs->ctx && bind(rxs->ctx) == ICS_OK) (void)hipFree(rxs->d_ring);  // waits for the device
  rxs->d_ring = nullptr;
}

// The plan's list to the device on `st`: *d_list is valid for the launch the
// caller enqueues next, which lease_done() marks.  Holds pa.mu in between.
struct PieceLease {
  PieceLease(PieceArea& pa, const std::vector<ics_copy_piece>& list, hipStream_t st)
      : lock_(pa.mu), s_(pa.slot[pa.next]), st_(st) {
    pa.next = (pa.next + 1) % PieceArea::kSlots;
    const size_t bytes = list.size() * sizeof(ics_copy_piece);
    if (!s_.ev) err_ = hipEventCreateWithFlags(&s_.ev, hipEventDisableTiming);
    if (err_ == hipSuccess && s_.used) err_ = hipEventSynchronize(s_.ev);  // the launch kSlots calls ago
    if (err_ != hipSuccess) return;
    s_.used = false;
    if (bytes > s_.cap) {
      if (s_.h) (void)hipHostFree(s_.h);
      if (s_.d) (void)hipFree(s_.d);
      s_.h = s_.d = nullptr;
      s_.cap = 0;
      const size_t cap = std::max<size_t>((bytes + (bytes >> 1) + 65535) & ~size_t(65535), size_t(1) << 16);
      err_ = hipHostMalloc(&s_.h, cap, hipHostMallocDefault);
      if (err_ == hipSuccess) err_ = hipMalloc(&s_.d, cap);
      if (err_ != hipSuccess) return;
      s_.cap = cap;
    }
    std::memcpy(s_.h, list.data(), bytes);
    err_ = hipMemcpyAsync(s_.d, s_.h, bytes, hipMemcpyHostToDevice, st);
  }
  ~PieceLease() {
    if (err_ != hipSuccess || !s_.d) return;
    if (hipEventRecord(s_.ev, st_) == hipSuccess) {
      s_.used = true;
    } else {  // cannot track this call's use: wait for it here
      (void)hipStreamSynchronize(st_);
    }
  }
  hipError_t error() const { return err_; }
  const void* d_list() const { return s_.d; }

 private:
  std::lock_guard<std::mutex> lock_;
  PieceArea::Slot& s_;
  hipStream_t st_;
  hipError_t err_ = hipSuccess;
};

}  // namespace

extern "C" {

int ics_rx_stream_create(ics_ctx* ctx, uint64_t capacity, ics_rx_stream** out) {
  if (!out) return fail(ICS_ERR_INVALID, "null output pointer");
  *out = nullptr;
  if (int rc = bind(ctx)) return rc;
  ics_rx_stream* rxs = nullptr;
  if (int rc = ics_rx_stream_create_host(capacity, &rxs)) return rc;
  if (hipError_t e = hipMalloc(&rxs->d_ring, size_t(capacity))) {
    rxs->d_ring = nullptr;
    (void)ics_rx_stream_destroy(rxs);
    return hip_fail(e, "ring allocation");
  }
  rxs->ctx = ctx;
  rxs->free_ring = free_ring;
  *out = rxs;
  return ICS_OK;
}

int ics_rx_stream_ring(ics_rx_stream* rxs, void** d_ring) {
  if (!rxs || !d_ring) return fail(ICS_ERR_INVALID, "null argument");
  if (!rxs->d_ring) return fail(ICS_ERR_INVALID, "stream without a ring (ics_rx_stream_create_host)");
  *d_ring = rxs->d_ring;
  return ICS_OK;
}

int ics_rx_stream_receive_batch(ics_ctx* ctx, ics_rx_stream* rxs, const void* d_dgrams, const uint64_t* h_offsets,
                                uint64_t stride, uint64_t dgram_len, uint64_t n, const ics_tcp_rx* h_recs,
                                const uint8_t* h_take, void* stream) {
  if (int rc = bind(ctx)) return rc;
  if (!rxs) return fail(ICS_ERR_INVALID, "null stream");
  if (!rxs->d_ring) return fail(ICS_ERR_INVALID, "stream without a ring (ics_rx_stream_create_host)");
  if (rxs->ctx != ctx) return fail(ICS_ERR_INVALID, "stream of another context");
  if (n == 0) return ICS_OK;
  if (!h_recs) return fail(ICS_ERR_INVALID, "null records");
  if (!d_dgrams) return fail(ICS_ERR_INVALID, "null datagram buffer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(rxs->mu);
  // on a copy of the state, committed once the copy is enqueued: an argument
  // error, an allocation failure or a HIP error leaves the stream as it was
  try {
    icsum::rx::State w = rxs->st;
    if (int rc = icsum::rx::run_plan(w, rxs->plan, h_recs, n, h_take, h_offsets, stride, dgram_len)) return rc;
    const uint64_t m = rxs->plan.size();
    if (m) {
      const uint64_t src_bytes = h_offsets ? h_offsets[n] : (n - 1) * stride + dgram_len;
      int rc;
      {
        PieceLease lease(ctx->rx_pieces, rxs->plan, st);
        ICS_HIP(lease.error());
        rc = copy_pieces_device(ctx, d_dgrams, src_bytes, rxs->d_ring, w.capacity, lease.d_list(), m, st);
      }
      if (rc != ICS_OK) return rc;
    }
    rxs->st = std::move(w);
    return m ? bounds_verdict(st, ICS_OK) : ICS_OK;
  } catch (const std::bad_alloc&) {
    return fail(ICS_ERR_NOMEM, "receive stream plan: out of host memory");
  }
}

int ics_rx_stream_read(ics_ctx* ctx, ics_rx_stream* rxs, void* h_dst, uint64_t len, uint64_t* got, void* stream) {
  if (int rc = bind(ctx)) return rc;
  if (!rxs || !got) return fail(ICS_ERR_INVALID, "null argument");
  if (!rxs->d_ring) return fail(ICS_ERR_INVALID, "stream without a ring (ics_rx_stream_create_host)");
  if (rxs->ctx != ctx) return fail(ICS_ERR_INVALID, "stream of another context");
  if (!h_dst && len) return fail(ICS_ERR_INVALID, "null destination");
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t off[2], have[2], ranges = 0;
  if (int rc = ics_rx_stream_peek(rxs, off, have, &ranges)) return rc;
  uint64_t done = 0;
  for (uint32_t k = 0; k < ranges && done < len; ++k) {
    const uint64_t take = std::min<uint64_t>(have[k], len - done);
    ICS_HIP(hipMemcpyAsync(static_cast<uint8_t*>(h_dst) + done, static_cast<const uint8_t*>(rxs->d_ring) + off[k],
                           size_t(take), hipMemcpyDeviceToHost, st));
    done += take;
  }
  ICS_HIP(hipStreamSynchronize(st));
  if (int rc = ics_rx_stream_pop(rxs, done)) return rc;
  *got = done;
  return ICS_OK;
}

}  // extern "C"
