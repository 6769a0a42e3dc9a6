// batch.h — batch entry points of the drop-in types, backed by the MI355X
// engine (libicsum.so, include/icsum.h).  These are the calls a busy stack
// makes instead of one compute_checksum()/parse() per object:
//
//   checksum()            InternetChecksum{init_i}.add(seg_i).value()     checksum.h:17-41
//   compute_checksums()   TCPSegment::compute_checksum(pseudo) per pair    tcp_segment.cpp:109-118
//                         IPv4Header::compute_checksum() per header        ipv4_header.cpp:113-123
//   verify_raw()          IPv4Header::parse + TCPSegment::parse checks     ipv4_header.cpp:9-59, tcp_segment.cpp:11-65
//   wrap()                TCPOverIPv4Adapter::wrap_tcp_in_ip per message   tcp_over_ip.cpp:69-88
//                         (headers + both checksums serialized on the GPU;
//                         payloads copied once, into the DMA arena)
//   unwrap()/unwrap_raw() TCPOverIPv4Adapter::unwrap_tcp_in_ip per datagram tcp_over_ip.cpp:10-67
//   unwrap_records()      the same from the device's ics_tcp_rx records (fields parsed on the GPU)
//   receive_records()     unwrap_records' gates, then TCPReceiver::receive per accepted message
//                         into an icsum::RxStream whose bytes stay in device memory
//                         (tcp_receiver.cpp:4-44, reassembler.cpp:4-103, byte_stream.cpp:60-67)
//
// Results are bit-identical to the per-object calls.  All checksum arithmetic
// runs on the GPU; a BatchEngine cannot be constructed without one (there is
// no silent CPU fallback).  One engine per thread, or guard it externally.
#ifndef ICSUM_HOST_BATCH_H
#define ICSUM_HOST_BATCH_H

#include <cstdint>
#include <memory>
#include <optional>
#include <span>
#include <string>
#include <string_view>
#include <vector>

#include "icsum.h"
#include "ipv4_datagram.h"
#include "ipv4_header.h"
#include "tcp_over_ip.h"
#include "tcp_segment.h"

namespace icsum {

namespace detail {
class WorkerPool;  // par_for.h
}

// The fields wrap_tcp_in_ip puts on the wire for `msg` from an adapter with
// configuration `cfg` (tcp_over_ip.cpp:71-80, tcp_segment.cpp:76-106): the
// record the device-side wrap (ics_tcp_wrap_batch) serializes.
ics_tcp_msg wrap_fields(const FdAdapterConfig& cfg, const TCPMessage& msg);

class BatchEngine;

// One connection's receive stream (ics_rx_stream, include/icsum.h): the state
// of TCPReceiver + Reassembler + ByteStream's writer on the host, the bytes in
// a ring on the engine's device.  RxStream(capacity) alone is the CPU-only
// object (plan and the queries); with an engine it has its ring and refers to
// the engine's context: destroy it before the BatchEngine.
class RxStream
{
  public:
    explicit RxStream(uint64_t capacity);
    RxStream(BatchEngine& eng, uint64_t capacity);
    ~RxStream();
    RxStream(const RxStream&) = delete;
    RxStream& operator=(const RxStream&) = delete;

    ics_rx_stream* get() const { return rxs_; }
    TCPReceiverMessage send() const;  // TCPReceiver::send
    ics_rx_stats_t stats() const;
    // ics_rx_stream_plan over host records (CPU-only path): the batch's copy list
    std::vector<ics_copy_piece> plan(std::span<const ics_tcp_rx> recs, const uint8_t* take, const uint64_t* offsets,
                                     uint64_t stride = 0, uint64_t dgram_len = 0);
    // the ring ranges (offset, length) that hold the buffered bytes, in stream order
    std::vector<std::pair<uint32_t, uint32_t>> peek() const;
    void pop(uint64_t len);  // Reader::pop; throws beyond bytes_buffered
    void set_error();        // reader().set_error()
    std::string read(uint64_t len);  // read(reader, len, out) from the device ring (needs an engine)

  private:
    ics_rx_stream* rxs_ = nullptr;
    ics_ctx* ctx_ = nullptr;
};

class BatchEngine
{
  public:
    explicit BatchEngine(int device = 0);  // throws std::runtime_error without a usable GPU
    ~BatchEngine();
    BatchEngine(const BatchEngine&) = delete;
    BatchEngine& operator=(const BatchEngine&) = delete;

    std::vector<uint16_t> checksum(std::span<const std::string_view> segs, std::span<const uint32_t> init = {});
    void compute_checksums(std::span<TCPSegment> segs, std::span<const IPv4Header> hdrs);
    void compute_checksums(std::span<IPv4Header> hdrs);
    // ICS_ST_* status bits per raw wire datagram (ICS_ST_ACCEPT = all parse checks pass)
    std::vector<uint8_t> verify_raw(std::span<const std::string_view> wires);
    std::vector<InternetDatagram> wrap(TCPOverIPv4Adapter& adapter, std::span<const TCPMessage> msgs);
    // the same, consuming the messages: each payload string is moved into its
    // datagram after the one copy into the arena
    std::vector<InternetDatagram> wrap(TCPOverIPv4Adapter& adapter, std::vector<TCPMessage>&& msgs);
    std::vector<std::optional<TCPMessage>> unwrap(TCPOverIPv4Adapter& adapter,
                                                  std::span<const InternetDatagram> dgrams);
    std::vector<std::optional<TCPMessage>> unwrap_raw(TCPOverIPv4Adapter& adapter,
                                                      std::span<const std::string_view> wires);

    // the same operations on an already packed batch (bytes + n+1 offsets),
    // e.g. a DatagramBatch arena in page-locked memory: no packing copy
    std::vector<uint8_t> verify_packed(const uint8_t* bytes, const uint64_t* offsets, size_t n);
    void patch_packed(uint8_t* bytes, const uint64_t* offsets, size_t n);  // compute + store both checksums
    // device-side wrap of a packed batch: datagram i = [40 B room][payload i],
    // headers + both checksums written into `bytes` (ics_tcp_wrap_batch_host)
    void wrap_packed(uint8_t* bytes, const uint64_t* offsets, const ics_tcp_msg* msgs, size_t n);
    std::vector<std::optional<TCPMessage>> unwrap_packed(TCPOverIPv4Adapter& adapter, const uint8_t* bytes,
                                                         const uint64_t* offsets, size_t n);
    // the same results from the device's message records
    // (ics_tcp_unwrap_batch_host: one 40-byte ics_tcp_rx per datagram, no host
    // pass over the headers): the adapter's gates applied from record fields
    // in datagram order, one payload copy per accepted datagram
    std::vector<std::optional<TCPMessage>> unwrap_records(TCPOverIPv4Adapter& adapter, const uint8_t* bytes,
                                                          const uint64_t* offsets, size_t n);

    // Receive path with the bytes left on the device: the datagrams are in
    // device memory (d_dgrams, packed by the n + 1 HOST offsets).  The message
    // records are parsed there (ics_tcp_unwrap_batch), unwrap_records' gates run
    // on the host from record fields in datagram order, and every accepted
    // message is received into `rx` (ics_rx_stream_receive_batch): its state is
    // final on return, its bytes follow on the engine's stream.  No payload
    // string is ever built.  Returns the number of accepted datagrams; `take`
    // (optional, n bytes) receives which.
    size_t receive_records(TCPOverIPv4Adapter& adapter, RxStream& rx, const void* d_dgrams, const uint64_t* offsets,
                           size_t n, uint8_t* take = nullptr);

    // the resident tick server (ics_set_tick_server): a per-tick loop's calls
    // of <= 16 x blocks datagrams without a kernel launch each; 0 turns it
    // off; blocks 1..8 (ics_set_tick_server_blocks, default 4)
    void set_tick_server(uint32_t idle_us);
    void set_tick_server_blocks(uint32_t blocks);

    // page-locked host memory from the engine's device runtime
    void* host_alloc(size_t bytes);
    void host_free(void* p);

    int device() const { return device_; }
    ics_ctx* context() const { return ctx_; }  // for the C-ABI calls this class does not wrap

  private:
    template <typename Msgs, typename Take>
    std::vector<InternetDatagram> wrap_impl(const TCPOverIPv4Adapter& adapter, Msgs& msgs, Take take_payload);
    uint8_t* scratch(size_t bytes);  // page-locked arena reused across calls
    template <typename Fn>
    void ranges(size_t n, Fn&& fn);  // fn(i0, i1) over [0, n) on up to 8 of the engine's threads
    template <typename Len, typename Put>
    std::vector<uint64_t> pack(size_t n, Len len, Put put);  // n items into scratch(), offsets back

    ics_ctx* ctx_ = nullptr;
    int device_ = 0;
    uint8_t* scratch_ = nullptr;
    size_t scratch_cap_ = 0;
    void* d_rx_ = nullptr;  // receive_records: device room for the offsets and the records, grown on demand
    size_t d_rx_cap_ = 0;
    std::unique_ptr<detail::WorkerPool> pool_{};  // ranges()' workers, started on first use
};

}  // namespace icsum

#endif
