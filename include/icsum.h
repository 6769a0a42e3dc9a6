/*
 * icsum.h — C-ABI of the MI355X Internet-checksum engine (libicsum.so).
 *
 * This is the drop-in boundary for the one per-byte transform the reference
 * stack (qmmzzdx/tcpip_network_protocol_stack) implements itself: the RFC-1071
 * one's-complement 16-bit sum over IPv4 headers and TCP segments.  Every entry
 * point below replaces a batch of calls to a reference C++ routine; the
 * reference has no C ABI of its own (its "interface" is the C++ header surface,
 * SURVEY.md §8b), so each declaration cites the reference function whose
 * semantics it reproduces bit for bit.
 *
 * Conventions
 *   - All functions return ICS_OK (0) or a negative ICS_ERR_* code.  No C++
 *     exception ever crosses this boundary; the message of the last failure on
 *     the calling thread is available from ics_last_error().
 *   - d_* pointers are device (HBM) pointers on the context's GPU; h_* pointers
 *     are host pointers.  `stream` is a hipStream_t (NULL = the legacy default
 *     stream of the context's device).  Device-pointer calls are asynchronous
 *     with respect to the host: they enqueue on `stream` and return.
 *   - Segment addressing (used by every batch call):
 *       d_offsets != NULL : segment i = bytes[d_offsets[i], d_offsets[i+1])
 *                           (n+1 monotone uint64 offsets; starts may be odd /
 *                           unaligned — byte roles are relative to each start;
 *                           the *_host calls reject decreasing h_offsets with
 *                           ICS_ERR_INVALID, the device calls trust them and
 *                           libicsum_debug.so reports them)
 *       d_offsets == NULL : segment i = bytes[i*stride, i*stride + seg_len)
 *   - Byte bases (d_bytes, d_dgrams, d_payloads, h_bytes, ...) may lie at ANY
 *     address, as InternetChecksum::add takes any string_view
 *     (util/tools/checksum.h:20-28): e.g. the IPv4 datagrams of a frame arena
 *     14 bytes in.  Loads stay inside the 16-byte-aligned blocks that hold a
 *     segment's bytes (never outside the pages of the batch).  Only the
 *     record arrays d_msgs / d_hdrs must be 4-byte aligned (ICS_ERR_INVALID
 *     otherwise); fixed stride == length == 64 B runs the dense kernel only
 *     from a 16-byte-aligned base (same results either way).
 *   - A context is bound to one device and may be used from several host
 *     threads (launch calls are thread-safe; the host-memory *_host calls
 *     serialise on an internal staging lock).
 */
#ifndef ICSUM_H
#define ICSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICS_ABI_VERSION 2 /* 2: ics_dispatch_info_t gained the host-pipeline counters */

/* ---- status codes ------------------------------------------------------ */
#define ICS_OK 0
#define ICS_ERR_INVALID (-1)     /* bad argument (null pointer, bad mode, ...) */
#define ICS_ERR_HIP (-2)         /* HIP runtime error (message has details) */
#define ICS_ERR_NOMEM (-3)       /* device / pinned allocation failed */
#define ICS_ERR_NODEVICE (-4)    /* no GPU / device index out of range */

/* ---- per-datagram status bits written by ics_ipv4_tcp_batch ------------ */
/* IPv4Header::parse success: ver==4, hlen>=5, recomputed == given
 * (util/ipv4_header/ipv4_header.cpp:9-59).  In COMPUTE/PATCH mode: ver==4 &&
 * hlen>=5 only (nothing to compare). */
#define ICS_ST_IPV4_OK 0x01u
/* TCP checksum: VERIFY = InternetChecksum{pseudo}.add(all bytes after the IPv4
 * header).value()==0 (util/tcp_segment/tcp_segment.cpp:11-18);
 * COMPUTE/PATCH = the TCP checksum field lies inside the datagram (patchable). */
#define ICS_ST_TCP_CKSUM_OK 0x02u
/* TCP header parse: >=20 bytes after the IPv4 header and data offset >= 5
 * (tcp_segment.cpp:25-65). */
#define ICS_ST_TCP_HDR_OK 0x04u
/* proto == IPv4Header::PROTO_TCP (util/tcp_over_ip/tcp_over_ip.cpp:26-29). */
#define ICS_ST_PROTO_TCP 0x08u
/* all of the above: the datagram would pass unwrap_tcp_in_ip's parse steps. */
#define ICS_ST_ACCEPT 0x0Fu

/* ---- modes of ics_ipv4_tcp_batch ---------------------------------------- */
#define ICS_MODE_COMPUTE 0 /* IPv4Header::compute_checksum + TCPSegment::compute_checksum */
#define ICS_MODE_VERIFY 1  /* IPv4Header::parse + TCPSegment::parse checksum checks */
#define ICS_MODE_PATCH 2   /* COMPUTE, then write both checksum fields in place */

typedef struct ics_ctx ics_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
const char* ics_version(void);
int ics_abi_version(void);
int ics_device_count(int* count);
/* One context per GPU.  Allocates the context's staging resources lazily. */
int ics_create(int device, ics_ctx** out);
int ics_destroy(ics_ctx* ctx);
int ics_device_of(const ics_ctx* ctx, int* device);
/* Message of the last failing call made by this thread ("" if none). */
const char* ics_last_error(void);

/* ---- a1-a4: InternetChecksum over a batch of segments ------------------ */
/* d_out[i] = InternetChecksum{init_i}.add(segment_i).value()
 *   replaces util/tools/checksum.h:17 (ctor), :20-28 (add), :31-41 (value);
 *   the TCP use is util/tcp_segment/tcp_segment.cpp:109-118 with init_i =
 *   IPv4Header::pseudo_checksum() (ipv4_header.cpp:103-110).
 * d_init == NULL means init_i = 0.  Bit-exact for every length, including the
 * reference's uint32 wrap above 131074 bytes of 0xFF. */
int ics_checksum_batch(ics_ctx* ctx, const void* d_bytes, const uint64_t* d_offsets,
                       uint64_t stride, uint64_t seg_len, const uint32_t* d_init,
                       uint16_t* d_out, uint64_t n, void* stream);

/* Unfolded running sum, for multi-piece add() chains (checksum.h:44-59, parity
 * carried across pieces): d_sum[i] = sum_ after InternetChecksum{init_i} has
 * had add(segment_i) applied with parity_ = d_odd[i] (0/1; NULL = all 0).
 * Chain pieces by feeding d_sum back as d_init and (len & 1) ^ odd as d_odd;
 * fold with ics_fold_batch or on the host. */
int ics_sum_batch(ics_ctx* ctx, const void* d_bytes, const uint64_t* d_offsets,
                  uint64_t stride, uint64_t seg_len, const uint32_t* d_init,
                  const uint8_t* d_odd, uint32_t* d_sum, uint64_t n, void* stream);

/* Dispatch of offsets batches (d_offsets != NULL) in ics_checksum_batch /
 * ics_sum_batch.  BINNED measures the length mix on the device and a one-block
 * plan kernel picks, per batch: split into length bins (each run with the lane
 * geometry that suits it), or the whole batch in one launch with 64/32-lane
 * groups (long segments dominate), 16-lane groups (short and MTU-sized) or
 * the small-segment body (ACK-sized);
 * SINGLE runs one launch with the long-segment geometry.  AUTO (default) =
 * BINNED for batches of >= 65536 segments.  Results are identical; only the
 * speed differs.  Per context; not a reference interface. */
#define ICS_BINNING_AUTO (-1)
#define ICS_BINNING_SINGLE 0
#define ICS_BINNING_BINNED 1
int ics_set_binning(ics_ctx* ctx, int mode);

/* d_out[i] = InternetChecksum::value() of a raw sum (checksum.h:31-41). */
int ics_fold_batch(ics_ctx* ctx, const uint32_t* d_sum, uint16_t* d_out, uint64_t n,
                   void* stream);

/* ---- a7/a8/a10/a11/a13: fused IPv4 + TCP over raw datagrams ------------- */
/* Each segment is one raw IPv4 datagram (wire bytes, header first).  Per
 * datagram, in one pass over its bytes:
 *   ip_ck  = IPv4Header::compute_checksum() of the parsed fields
 *            (ipv4_header.cpp:113-123: 20 serialized bytes, cksum=0, flag bit
 *            0x8000 dropped, options never summed)
 *   pseudo = IPv4Header::pseudo_checksum() (ipv4_header.cpp:103-110)
 *   tcp_ck = COMPUTE/PATCH: TCPSegment::compute_checksum(pseudo) over the bytes
 *            after the IPv4 header with the TCP checksum field read as 0
 *            (tcp_segment.cpp:109-118)
 *            VERIFY: InternetChecksum{pseudo}.add(all bytes after the IPv4
 *            header).value() (tcp_segment.cpp:11-18; 0 means valid)
 *   status = ICS_ST_* bits above.
 * PATCH additionally stores ip_ck / tcp_ck big-endian into the datagram
 * (the checksum fields wrap_tcp_in_ip fills, tcp_over_ip.cpp:69-88).
 * Datagrams shorter than 20 bytes get ip_ck = tcp_ck = status = 0.
 * Any of d_ip_ck / d_tcp_ck / d_status may be NULL. */
int ics_ipv4_tcp_batch(ics_ctx* ctx, void* d_dgrams, const uint64_t* d_offsets,
                       uint64_t stride, uint64_t dgram_len, uint64_t n, int mode,
                       uint16_t* d_ip_ck, uint16_t* d_tcp_ck, uint8_t* d_status,
                       void* stream);

/* ---- router forwarding batch (src/router/router.cpp:43-50) -------------- */
/* For each raw datagram whose IPv4 header parses (ver 4, hlen>=5, checksum
 * valid): if ttl <= 1 the datagram is dropped (d_status[i] = 0, bytes
 * untouched); else ttl-- and the header checksum is recomputed with
 * IPv4Header::compute_checksum() semantics and written in place
 * (d_status[i] = 1).  Unparseable datagrams get d_status[i] = 0. */
int ics_router_ttl_batch(ics_ctx* ctx, void* d_dgrams, const uint64_t* d_offsets,
                         uint64_t stride, uint64_t dgram_len, uint64_t n,
                         uint8_t* d_status, void* stream);

/* The same router step with the forwarded headers apart: the datagrams are
 * only read, and the 20 bytes Router::route's send_datagram serializes as the
 * header piece (router.cpp:39-66 -> ipv4_header.cpp:62-86: ttl - 1, the
 * recomputed checksum, the reserved flag bit dropped, no options) go to
 * d_hdrs + 20 * i, 4-byte aligned, one coalesced array.  Datagram i on the
 * wire = d_hdrs[20 i .. 20 i + 20) followed by its payload piece, the bytes
 * after the parsed header: [start + 4 hlen, end) (ipv4_header.cpp:50).
 * d_status[i] as ics_router_ttl_batch; a dropped or unparseable datagram's 20
 * header bytes are zero.  A forwarded header equals the first 20 bytes the
 * in-place call leaves. */
int ics_router_ttl_headers(ics_ctx* ctx, const void* d_dgrams, const uint64_t* d_offsets,
                           uint64_t stride, uint64_t dgram_len, uint64_t n, void* d_hdrs,
                           uint8_t* d_status, void* stream);

/* ---- route lookup (src/router/router.cpp:15-24 add_route, :77-87 match) -- */
/* A route table with Router::match's exact semantics.  The table functions
 * need no context and no GPU.  add(prefix, L, ...) stores the route under
 * (L, rotr(prefix, 32 - L)), a later add with the same (L, prefix) replacing
 * the earlier one; match(addr) tries L = 31 down to 0 with addr >> (32 - L)
 * and the first hit wins.  What follows from that is reproduced bit for bit:
 *   - a route whose prefix has a bit set below its top L bits (L = 0: any bit)
 *     is accepted and can never match ("dead");
 *   - bit 0 of the address never takes part (the longest length tried is 31);
 *   - the answer's next hop is next_hop.value_or(dst): the address looked up
 *     for a direct route, and a present next hop of 0.0.0.0 is NOT direct.
 * The one deliberate difference: prefix_len 32 indexes past the reference's
 * 32-entry array (undefined behaviour there); here prefix_len > 31 is
 * ICS_ERR_INVALID.  iface is the reference's interface_num and must be below
 * 2^31.  A table is guarded by a mutex (concurrent matches are allowed) and
 * is compiled, on the first match or device use after a change, into the
 * flat 16-8-7 trie the device reads; ICS_ERR_NOMEM if that
 * image would reach 2^31 words.  A table belongs to the library that created
 * it (libicsum.so or libicsum_debug.so). */
typedef struct ics_route_table ics_route_table;
typedef struct ics_route_stats_t {
  uint64_t routes_added;  /* adds since create / clear */
  uint64_t routes_live;   /* ... of them, those whose prefix can match */
  uint64_t routes_dead;   /* ... and those that never can */
  uint64_t route_records; /* distinct live (prefix_len, prefix): the image's route records */
  uint64_t image_words;   /* trie words: 65536 + 256 l2_chunks + 128 l3_chunks */
  uint64_t l2_chunks;     /* 256-word chunks (routes longer than /16 under a /16) */
  uint64_t l3_chunks;     /* 128-word chunks (routes longer than /24 under a /24) */
} ics_route_stats_t;
int ics_route_table_create(ics_route_table** out);
int ics_route_table_destroy(ics_route_table* tbl);
int ics_route_table_add(ics_route_table* tbl, uint32_t prefix, uint32_t prefix_len, uint32_t iface,
                        int has_next_hop, uint32_t next_hop);
int ics_route_table_clear(ics_route_table* tbl);
/* 1: matched (*iface, *next_hop set; either may be NULL), 0: no route
 * (*iface = 0xFFFFFFFF, *next_hop = 0), negative: error.  Walks the same
 * compiled image the device reads. */
int ics_route_table_match(ics_route_table* tbl, uint32_t addr, uint32_t* iface, uint32_t* next_hop);
int ics_route_table_stats(ics_route_table* tbl, ics_route_stats_t* stats);

/* d_iface[i], d_next_hop[i] = match(d_addrs[i]) for n host-order addresses,
 * one lane each (k_route_lookup); no route: 0xFFFFFFFF and 0.  Either output
 * may be NULL.
 * Device image (all three calls below): the context keeps the images of a few
 * tables (least recently used replaced) and uploads a table's image on
 * `stream` on its first use after a change; that upload synchronises
 * `stream`, every other call only enqueues.  Calls on one stream see table
 * changes in order.  A launch already enqueued, on any stream, keeps the
 * image it was given: the upload that replaces an image (a changed table, or
 * another table taking its place) first waits for every such launch.  Calls
 * that read an unchanged image never wait for each other. */
#define ICS_NO_ROUTE 0xFFFFFFFFu
int ics_route_lookup_batch(ics_ctx* ctx, ics_route_table* tbl, const uint32_t* d_addrs, uint64_t n,
                           uint32_t* d_iface, uint32_t* d_next_hop, void* stream);

/* Router::route whole (router.cpp:27-70): ics_router_ttl_batch's step, then
 * match(header.dst) for every datagram that forwards — the ttl decrement and
 * checksum recompute come first, so a datagram with no route has been
 * rewritten (and is then dropped by the caller).  d_status[i] bits:
 * ICS_RT_FORWARD is ics_router_ttl_batch's status 1, and the bytes written
 * are exactly that call's, route or no route; ICS_RT_ROUTED: forwarded and a
 * route matched, d_iface[i] / d_next_hop[i] = the egress interface and
 * next_hop.value_or(dst).  Without ROUTED they are 0xFFFFFFFF and 0.
 * d_iface / d_next_hop may be NULL independently.  The lookup runs inside the
 * router kernel, on the dst it already holds: prefer these calls to the bare
 * step followed by ics_route_lookup_batch (1 M x 1500 B, headers apart: 41-51
 * us fused against 45-63 us as two launches and 33-34 us for the bare step,
 * from a 264 KiB to a 42 MB image). */
#define ICS_RT_FORWARD 0x01u
#define ICS_RT_ROUTED 0x02u
int ics_router_route_batch(ics_ctx* ctx, ics_route_table* tbl, void* d_dgrams, const uint64_t* d_offsets,
                           uint64_t stride, uint64_t dgram_len, uint64_t n, uint8_t* d_status,
                           uint32_t* d_iface, uint32_t* d_next_hop, void* stream);
/* The same with the forwarded headers apart, as ics_router_ttl_headers:
 * d_hdrs and (d_status & ICS_RT_FORWARD) are exactly that call's. */
int ics_router_route_headers(ics_ctx* ctx, ics_route_table* tbl, const void* d_dgrams,
                             const uint64_t* d_offsets, uint64_t stride, uint64_t dgram_len, uint64_t n,
                             void* d_hdrs, uint8_t* d_status, uint32_t* d_iface, uint32_t* d_next_hop,
                             void* stream);

/* ---- Ethernet frames through the hop (src/network_interface/network_interface.cpp) */
/* A neighbour table: the control half of the router's NetworkInterfaces —
 * each interface's addresses (the constructor's), its ARP cache
 * (arp_addr_table_) and its pending requests (arp_requests_), with the
 * reference's semantics bit for bit:
 *   - the cache is PER INTERFACE: a mapping learned on interface 0 is
 *     invisible on interface 1;
 *   - recv_frame's destination filter passes exactly two addresses, broadcast
 *     and the interface's own (multicast is dropped);
 *   - an ARP message parses iff its payload has at least 28 bytes and
 *     supported() holds (hardware type 1, protocol 0x0800, sizes 6 and 4,
 *     opcode 1 or 2); trailing padding is fine;
 *   - every ARP that passes the filter and parses is learned from, whoever
 *     its target is; a re-learn overwrites the address and resets the timer;
 *   - only a REPLY releases waiting datagrams; a REQUEST from an awaited
 *     address learns it and releases nothing; the pending-request entry is
 *     not erased by the reply;
 *   - tick: every timer += ms, a mapping is erased when its timer > 30000, a
 *     pending request when > 5000 (strict: 30000 and 5000 survive).  The
 *     request timer is the reference's uint32_t (it wraps), the mapping timer
 *     its size_t.
 * The queue of datagrams waiting for a reply (datagrams_waiting_) stays with
 * the CALLER, who owns their bytes: resolve() returning 0 means "hold it",
 * ICS_ARP_RELEASE means "those held for *sender_ip may go" (resolve again).
 * Deliberate differences:
 *   - the reference indexes _interfaces[n] unchecked; here an interface that
 *     was never given its addresses (set_iface) is never resolved (resolve
 *     returns 0 with no event, the device never sets ICS_FR_RESOLVED), and
 *     frames arriving on one get status 0 on the device and ICS_ERR_INVALID
 *     from ics_neigh_table_recv_frame;
 *   - a frame shorter than 14 bytes gets status 0 (the reference's app never
 *     hands such a frame to recv_frame).
 * The table functions need no context and no GPU.  A table is guarded by a
 * mutex, has an id and a generation that changes ONLY when its compiled
 * contents change — set_iface with new addresses, a learn that adds a mapping
 * or changes its address, a tick that erases a mapping; NOT a tick that only
 * ages timers, a pending request, or a re-learn of an identical mapping (that
 * resets the timer, which the image does not hold) — and is compiled lazily
 * into the image the device reads: one uint32 array,
 *   identity  4 words per interface 0 .. ifaces-1:
 *             mac[0..3] (as in memory), mac[4..5] | 0x10000 when configured, ip, 0
 *   slots     4 words each, a power-of-two count >= 2 x mappings (>= 4), open
 *             addressing with linear probing (wrapping) from
 *             hash(iface, ip) & (slots - 1):
 *             ip, iface | 0x80000000 (0: empty), mac[0..3], mac[4..5]
 * so every probe is one aligned 16-byte load and every probe sequence ends at
 * an empty slot.  A table belongs to the library that created it. */
typedef struct ics_neigh_table ics_neigh_table;
typedef struct ics_neigh_stats_t {
  uint64_t ifaces;           /* interfaces given their addresses */
  uint64_t mappings;         /* live ARP mappings over all interfaces */
  uint64_t pending_requests; /* ARP requests inside their 5 s hold-down */
  uint64_t image_ifaces;     /* identity entries of the image (highest interface used + 1) */
  uint64_t image_slots;      /* slots of the image's hash table */
  uint64_t generation;       /* changes only when the compiled contents change (see above) */
} ics_neigh_stats_t;
#define ICS_ALL_IFACES 0xFFFFFFFFu
#define ICS_ARP_REPLY 0x01u   /* recv_frame: the 42-byte reply frame was written, transmit it */
#define ICS_ARP_RELEASE 0x02u /* recv_frame: a REPLY arrived, datagrams held for *sender_ip may go */
#define ICS_ARP_REQUEST 0x04u /* resolve: the 42-byte broadcast request was written, transmit it */
int ics_neigh_table_create(ics_neigh_table** out);
int ics_neigh_table_destroy(ics_neigh_table* tbl);
/* NetworkInterface ctor: interface `iface` has this Ethernet and IPv4 address.  iface < 65536. */
int ics_neigh_table_set_iface(ics_neigh_table* tbl, uint32_t iface, const uint8_t mac[6], uint32_t ip);
/* arp_addr_table_.insert_or_assign(ip, AddrMapping(mac)) on one interface: timer back to 0. */
int ics_neigh_table_learn(ics_neigh_table* tbl, uint32_t iface, uint32_t ip, const uint8_t mac[6]);
/* 1 hit (mac written), 0 miss; walks the compiled image the device reads. */
int ics_neigh_table_lookup(ics_neigh_table* tbl, uint32_t iface, uint32_t ip, uint8_t mac[6]);
/* NetworkInterface::tick (network_interface.cpp:89-102) on one interface, or on all with ICS_ALL_IFACES. */
int ics_neigh_table_tick(ics_neigh_table* tbl, uint32_t iface, uint64_t ms);
/* recv_frame for ONE frame on the host (network_interface.cpp:40-87).  *status
 * gets the classification bits the kernels write (ICS_FR_FOR_US .. ICS_FR_DGRAM
 * below; never the routing bits).  For an ARP frame that parses: learns
 * sender_ip -> sender address, sets *sender_ip, and *events gets
 *   ICS_ARP_REPLY   - a request for this interface's ip: the reply is in reply42
 *   ICS_ARP_RELEASE - opcode REPLY
 * or 0.  All four outputs are required; `iface` must be configured. */
int ics_neigh_table_recv_frame(ics_neigh_table* tbl, uint32_t iface, const void* frame, size_t len,
                               uint8_t* status, uint32_t* events, uint32_t* sender_ip, void* reply42);
/* send_datagram's control half (network_interface.cpp:18-37).  Returns 1 and
 * writes the 14-byte header (dst = the neighbour, src = the interface, type
 * 0x0800); returns 0 on a miss, and then, if no request for that ip is
 * pending on the interface, writes the 42-byte broadcast ARP request to
 * request42, sets ICS_ARP_REQUEST in *events and starts the 5 s hold-down.
 * All three outputs are required. */
int ics_neigh_table_resolve(ics_neigh_table* tbl, uint32_t iface, uint32_t next_hop, uint8_t hdr14[14],
                            uint32_t* events, void* request42);
int ics_neigh_table_stats(ics_neigh_table* tbl, ics_neigh_stats_t* stats);

/* recv_frame's data-plane half for n Ethernet frames (k_frame<false>): frame i
 * arrived on interface in_iface, or d_in_iface[i] when that is non-NULL (a
 * ring fed from several fds).  d_status[i] bits: */
#define ICS_FR_RESOLVED 0x04u /* ics_router_frames only: ROUTED, the egress interface is configured and the next hop is in ITS cache */
#define ICS_FR_DGRAM 0x08u    /* IPV4 and IPv4Header::parse succeeds on the payload: what recv_frame queues */
#define ICS_FR_FOR_US 0x10u   /* >= 14 bytes, the ingress interface is configured, dst is broadcast or its address */
#define ICS_FR_IPV4 0x20u     /* FOR_US and type 0x0800 */
#define ICS_FR_ARP 0x40u      /* FOR_US and type 0x0806 */
#define ICS_FR_ARP_OK 0x80u   /* ARP and the message parses: hand the frame to ics_neigh_table_recv_frame */
/* The frames are only read; addressing (d_offsets / stride / frame_len, any
 * base address) as every batch call.  Uploads the table's image as the route
 * calls upload theirs (above). */
int ics_frame_recv_batch(ics_ctx* ctx, ics_neigh_table* neigh, const void* d_frames, const uint64_t* d_offsets,
                         uint64_t stride, uint64_t frame_len, uint64_t n, uint32_t in_iface,
                         const uint32_t* d_in_iface, uint8_t* d_status, void* stream);
/* The whole hop (k_frame<true>): recv_frame's classification, then for the
 * frames that carry a datagram exactly ics_router_route_headers on the
 * datagram at frame + 14 (ICS_RT_FORWARD, ICS_RT_ROUTED, d_iface, d_next_hop —
 * both nullable), then send_datagram's cache lookup on the egress interface
 * (ICS_FR_RESOLVED) and make_frame's header.  One 36-byte record per frame at
 * d_hdrs + 36 i, 4-byte aligned:
 *   [0,2)   zero (the pad that puts the IPv4 header on a dword boundary)
 *   [2,16)  the Ethernet header: neighbour's address, egress interface's, 0x0800
 *   [16,36) byte for byte ics_router_route_headers' 20 bytes
 * Frame i on the wire = d_hdrs[36 i + 2 .. 36 i + 36) followed by
 * [start + 14 + 4 hlen, end).  Without RESOLVED [0,16) is zero (the caller
 * holds the datagram and calls ics_neigh_table_resolve for the request);
 * without FORWARD all 36 bytes are zero.
 * Snapshot: the call resolves against the neighbour table AS OF THE CALL.  The
 * reference runs every recv_frame of a burst (learning) before route()
 * (sending); a caller who needs that order calls ics_frame_recv_batch, feeds
 * the ICS_FR_ARP_OK frames to ics_neigh_table_recv_frame, then calls this.
 * Measured (profiles/frame_hop.jsonl), 1 M x 1514 B, neighbour
 * tables of 1000 / 50 000 mappings: 69.6 / 71.3 us against 52 us for
 * ics_router_route_headers on the same datagrams at stride 1500 in the same
 * process; ics_frame_recv_batch 52 us against 44 us for the bare
 * ics_router_ttl_headers; the host loop this replaces, one
 * ics_neigh_table_resolve per datagram on 16 threads, 98-170 ms.  Why the
 * Ethernet layer costs what it does is supposed there, not profiled. */
int ics_router_frames(ics_ctx* ctx, ics_route_table* routes, ics_neigh_table* neigh, const void* d_frames,
                      const uint64_t* d_offsets, uint64_t stride, uint64_t frame_len, uint64_t n,
                      uint32_t in_iface, const uint32_t* d_in_iface, void* d_hdrs, uint8_t* d_status,
                      uint32_t* d_iface, uint32_t* d_next_hop, void* stream);

/* ---- a14 / §8(f) rank 2: device-side wrap_tcp_in_ip -------------------- */
/* The fields of one TCPMessage as TCPOverIPv4Adapter::wrap_tcp_in_ip
 * (util/tcp_over_ip/tcp_over_ip.cpp:69-88) puts them on the wire.  28 bytes. */
typedef struct ics_tcp_msg {
  uint32_t src, dst;   /* IPv4Header::src / dst, host order (FdAdapterConfig source / destination) */
  uint32_t seqno;      /* TCPSenderMessage::seqno, raw Wrap32 value */
  uint32_t ackno;      /* raw ackno; 0 when the message has none (tcp_segment.cpp:86) */
  uint16_t src_port, dst_port;
  uint16_t window;     /* TCPReceiverMessage::window_size */
  uint8_t flags;       /* ICS_TCP_* bits, as tcp_segment.cpp:92-97 derives them */
  uint8_t ttl;         /* IPv4Header::ttl (DEFAULT_TTL = 128 in wrap_tcp_in_ip) */
  uint16_t id;         /* IPv4Header::id (0 in wrap_tcp_in_ip) */
  uint16_t reserved;   /* 0 */
} ics_tcp_msg;
#define ICS_TCP_FIN 0x01u
#define ICS_TCP_SYN 0x02u
#define ICS_TCP_RST 0x04u /* sender.RST || receiver.RST */
#define ICS_TCP_ACK 0x10u /* receiver.ackno present */

/* Datagram i = bytes [off_i, off_i+1) (or fixed stride / dgram_len) holds 40
 * bytes of room for the headers followed by message i's payload, already in
 * place.  In one pass per datagram the engine sums the payload and writes the
 * serialized IPv4 header (ipv4_header.cpp:62-86: ver 4, hlen 5, tos 0,
 * len = datagram length mod 2^16, id, DF, ttl, proto 6, checksum, src, dst)
 * and TCP header (tcp_segment.cpp:76-106: ports, seqno, ackno, data offset 5,
 * flags, window, checksum, urgent 0) with both checksums
 * (TCPSegment::compute_checksum(pseudo_checksum()), then
 * IPv4Header::compute_checksum(), tcp_over_ip.cpp:83-84): the wire bytes of
 * serialize(wrap_tcp_in_ip(msg)), with no host-side serialization.
 * Datagrams shorter than 40 bytes are left untouched (checksums 0).
 * d_ip_ck / d_tcp_ck (optional) receive the two checksums. */
int ics_tcp_wrap_batch(ics_ctx* ctx, void* d_dgrams, const uint64_t* d_offsets, uint64_t stride,
                       uint64_t dgram_len, uint64_t n, const ics_tcp_msg* d_msgs, uint16_t* d_ip_ck,
                       uint16_t* d_tcp_ck, void* stream);

/* The same wrap with the headers kept apart — the two pieces an
 * InternetDatagram holds (util/tools/ipv4_datagram.h:10-34: header, then the
 * serialized segment) and what a writev/sendmmsg iovec pair sends: segment i
 * of d_payloads is message i's payload ALONE (no header room); the 40 header
 * bytes of datagram i go to d_hdrs + 40*i (4-byte aligned), written as one
 * coalesced array instead of into the payload stream.  Datagram i on the wire
 * = d_hdrs[40 i .. 40 i + 40) followed by payload i.  From 2^18 datagrams up
 * the engine runs two launches on `stream` (payload sums, then the headers),
 * faster than storing headers inside the payload stream;
 * d_msgs must be 4-byte aligned (both wrap calls). */
int ics_tcp_wrap_headers(ics_ctx* ctx, const void* d_payloads, const uint64_t* d_offsets, uint64_t stride,
                         uint64_t payload_len, uint64_t n, const ics_tcp_msg* d_msgs, void* d_hdrs,
                         uint16_t* d_ip_ck, uint16_t* d_tcp_ck, void* stream);

/* ---- device-side unwrap_tcp_in_ip: message records from a datagram batch - */
/* The mirror of ics_tcp_wrap_headers: what TCPOverIPv4Adapter::unwrap_tcp_in_ip
 * (util/tcp_over_ip/tcp_over_ip.cpp:14-64) and TCPSegment::parse
 * (util/tcp_segment/tcp_segment.cpp:25-65) read out of a datagram's bytes, as
 * one 40-byte record per datagram.  Let L be the datagram's length and
 * `status` the byte ICS_MODE_VERIFY writes for it, bit for bit.  PARSED means
 * (status & 7) == 7: ICS_ST_IPV4_OK, ICS_ST_TCP_CKSUM_OK and ICS_ST_TCP_HDR_OK.
 *   - Not PARSED: the 36 bytes before `status` are zero.
 *   - PARSED: hl = 4 * hlen (20..60), and TCP_HDR_OK guarantees hl + 20 <= L.
 *     With T the byte at hl:
 *       msg.src, msg.dst   header bytes 12-15 and 16-19, host order
 *       msg.ttl, msg.id    header byte 8, header bytes 4-5
 *       msg.src_port       T[0..1]        msg.dst_port  T[2..3]
 *       msg.seqno          T[4..7]
 *       msg.ackno          T[8..11] if T[13] & 0x10, else 0 (tcp_segment.cpp:42-45
 *                          resets an absent ackno; :86 serializes it as 0)
 *       msg.flags          T[13] & 0x17, the ICS_TCP_* bits
 *       msg.window         T[14..15]      msg.reserved  0
 *       pay_off            min(hl + 4 * doff, L), doff = T[12] >> 4 (>= 5)
 *       pay_len            (L - pay_off) mod 2^32
 *   - Options that claim more than the datagram holds: the payload is empty,
 *     no error (Parser::remove_prefix stops at the end, util/tools/parser.h:54-68).
 *   - proto != 6 does not affect PARSED and the fields are filled:
 *     ICS_ST_PROTO_TCP in `status` is what unwrap_tcp_in_ip:26 gates on.
 *   - The adapter's gates (tcp_over_ip.cpp:14-23, 39-64: destination and source
 *     address, ports, the listening -> connected transition, sequential in
 *     batch order) stay with the caller; they need only record fields.
 *   - Round trip: for a PARSED datagram with hlen 5, tos 0, fragment field
 *     0x4000, proto 6 (what wrap_tcp_in_ip writes, tcp_over_ip.cpp:69-88),
 *     len == L mod 2^16, doff 5, urgent 0 and no flag bits outside 0x17,
 *     ics_tcp_wrap_headers on rec.msg and [pay_off, pay_off + pay_len)
 *     reproduces its first 40 wire bytes. */
typedef struct ics_tcp_rx {   /* 40 bytes; arrays of it 4-byte aligned */
  ics_tcp_msg msg;            /* exactly what ics_tcp_wrap_* takes (28 bytes) */
  uint32_t pay_off;           /* TCPSenderMessage::payload starts this many bytes into the datagram */
  uint32_t pay_len;           /* and has this many bytes */
  uint8_t status;             /* the ICS_ST_* byte ICS_MODE_VERIFY writes for this datagram */
  uint8_t reserved[3];        /* 0 */
} ics_tcp_rx;

/* One datagram on the host: no context, no GPU.  Computes both checksums
 * itself (ipv4_header.cpp:9-59, tcp_segment.cpp:11-18), so *out is the whole
 * record, status included.  dgram may be NULL only when len is 0. */
int ics_tcp_unwrap_one(const void* dgram, size_t len, ics_tcp_rx* out);

/* n datagrams on the device (addressing as ics_ipv4_tcp_batch): the VERIFY
 * pass of ics_ipv4_tcp_batch on `stream` — its status bytes to d_status, or
 * to context scratch when d_status is NULL — then k_tcp_unwrap on the same
 * stream, one lane per datagram, reading only the header blocks: two launches
 * (the tuned verify kernels are left as they are).  d_recs:
 * n records, 4-byte aligned.  The datagrams are only read. */
int ics_tcp_unwrap_batch(ics_ctx* ctx, const void* d_dgrams, const uint64_t* d_offsets, uint64_t stride,
                         uint64_t dgram_len, uint64_t n, ics_tcp_rx* d_recs, uint8_t* d_status, void* stream);

/* The same on host memory: the datagrams go to the device (or are read in
 * place when the batch is small and page-locked), only the 40-byte records
 * come back.  Synchronous. */
int ics_tcp_unwrap_batch_host(ics_ctx* ctx, const void* h_dgrams, const uint64_t* h_offsets, uint64_t stride,
                              uint64_t dgram_len, uint64_t n, ics_tcp_rx* h_recs);

/* ---- receive streams: TCPReceiver + Reassembler per batch ----------------- */
/* The in-order byte stream of one connection, kept in a ring in device memory:
 * what TCPReceiver::receive (src/tcp_receiver/tcp_receiver.cpp:4-44) ->
 * Reassembler::insert (src/reassembler/reassembler.cpp:4-103) -> Writer::push
 * (src/byte_stream/byte_stream.cpp:60-67) do with the payloads of a batch of
 * ics_tcp_rx records, without a payload byte crossing to the host.
 *   Control plane (host, sequential, exact; needs no context and no GPU): an
 * ics_rx_stream holds the reference's state without the bytes — capacity C, the
 * optional ISN, bytes_pushed (== first_unassembled_index_), bytes_popped,
 * eof_index (UINT64_MAX until a FIN sets it), the closed and error flags and
 * the ordered interval list, each interval with the list of source ranges its
 * bytes come from in place of interval_str.  receive of one record performs the
 * reference's statements in their order; what follows from that is reproduced
 * bit for bit:
 *   - an RST sets the error and returns; a set error makes every later receive
 *     return at once;
 *   - before the ISN is set a record without SYN is dropped; the first SYN's
 *     seqno becomes the ISN;
 *   - a SYN always inserts at stream index 0, whatever its seqno (a second SYN
 *     with another seqno too);
 *   - absseq = unwrap(seqno, isn, bytes_pushed + 1) with the reference's
 *     conversions (the raw difference as an int32_t, the sum as an int64_t,
 *     + 2^32 when negative); stream index absseq - 1, which for absseq == 0 (the
 *     ISN itself without SYN) is UINT64_MAX and is rejected by `>= eof_index`;
 *   - insert rejects on a closed stream, first >= eof_index, or first >=
 *     first_unassembled + available_capacity;
 *   - a FIN that passes those tests sets eof_index = first + length even when
 *     its range, clipped to [first_unassembled, first_unassembled + available),
 *     is empty (a FIN behind the window is rejected and sets nothing);
 *   - merging, against the interval before (`prev`) and those behind:
 *       touching intervals merge (prev.end >= new.beg);
 *       a new range wholly inside prev (prev.end > new.end) is discarded;
 *       otherwise the new range WINS its overlap with prev;
 *       a following interval that ends later KEEPS its overlap;
 *       a covered following interval is erased;
 *     where overlapping segments carry different bytes these rules decide byte
 *     by byte which source survives — there is no "overlaps must agree" contract;
 *   - intervals are pushed while their start equals first_unassembled, and the
 *     stream closes when first_unassembled >= eof_index.
 * The one deliberate difference: capacity must be 1 .. 2^30 (ICS_ERR_INVALID
 * otherwise): the ring is a device allocation.  Reader::pop beyond
 * bytes_buffered (undefined in the reference) is refused.
 *   Data plane: a batch's plan ends in a copy list; stream byte i lives at ring
 * offset i mod C, pending bytes included (they lie inside [popped, popped + C)). */
typedef struct ics_rx_stream ics_rx_stream;
typedef struct ics_copy_piece { /* 16 bytes */
  uint64_t src;               /* byte offset in the source (datagram) buffer */
  uint32_t dst;               /* byte offset in the destination (ring): stream index mod C */
  uint32_t len;               /* bytes; may be 0 */
} ics_copy_piece;
typedef struct ics_rx_send_t { /* TCPReceiver::send (tcp_receiver.cpp:47-67) */
  uint32_t has_ackno;         /* the ISN is set */
  uint32_t ackno;             /* wrap(bytes_pushed + 1 + closed, isn), raw; 0 without has_ackno */
  uint16_t window;            /* min(available_capacity, 65535) */
  uint8_t rst;                /* the stream's error flag */
  uint8_t reserved;
} ics_rx_send_t;
typedef struct ics_rx_stats_t {
  uint64_t capacity, bytes_pushed, bytes_popped, bytes_buffered;
  uint64_t bytes_pending;     /* Reassembler::bytes_pending */
  uint64_t available_capacity;
  uint64_t eof_index;         /* UINT64_MAX: none yet */
  uint64_t intervals;         /* pending intervals */
  uint32_t closed, error;
  uint32_t finished;          /* closed and nothing buffered (Reader::is_finished) */
  uint32_t has_isn;
} ics_rx_stats_t;
/* A stream object without a ring (the CPU-only path: ics_rx_stream_plan and the
 * queries below; the device calls refuse it). */
int ics_rx_stream_create_host(uint64_t capacity, ics_rx_stream** out);
/* ... and with its ring of `capacity` bytes on ctx's device.  Such a stream
 * refers to its context: destroy it BEFORE ics_destroy(ctx). */
int ics_rx_stream_create(ics_ctx* ctx, uint64_t capacity, ics_rx_stream** out);
int ics_rx_stream_destroy(ics_rx_stream* rxs);
/* receive over records 0 .. n-1 in order: take[i] != 0 selects record i; take
 * == NULL selects every record with (status & 7) == 7 and ICS_ST_PROTO_TCP.
 * Datagram i starts at h_offsets[i] (n + 1 host offsets) or at i * stride with
 * dgram_len bytes.  After the last record the batch's copy list is written:
 * every byte now held, pending or pushed, whose surviving source is a record of
 * this batch lies in exactly one piece, src = the datagram's start + pay_off +
 * the clip, dst = stream index mod C.  Pieces come in increasing stream index,
 * are split at the ring's wrap and maximal otherwise, and have pairwise
 * disjoint destinations; bytes an earlier batch left in the ring and that still
 * win are not copied again.  *m = the number of pieces.  pieces == NULL: a dry
 * run that only counts (the state is left as it was).  ICS_ERR_INVALID, with the
 * state and the outputs untouched: cap < *m would be needed, a taken record
 * whose pay_off + pay_len exceeds its datagram, decreasing offsets. */
int ics_rx_stream_plan(ics_rx_stream* rxs, const ics_tcp_rx* recs, uint64_t n, const uint8_t* take,
                       const uint64_t* h_offsets, uint64_t stride, uint64_t dgram_len, ics_copy_piece* pieces,
                       uint64_t cap, uint64_t* m);
int ics_rx_stream_send(ics_rx_stream* rxs, ics_rx_send_t* out);
int ics_rx_stream_stats(ics_rx_stream* rxs, ics_rx_stats_t* out);
/* Reader::pop; refused (ICS_ERR_INVALID) beyond bytes_buffered. */
int ics_rx_stream_pop(ics_rx_stream* rxs, uint64_t len);
/* The ring ranges that hold stream bytes [popped, pushed): *ranges = 0, 1 or 2,
 * range k = ring bytes [off[k], off[k] + len[k]), in stream order. */
int ics_rx_stream_peek(ics_rx_stream* rxs, uint32_t off[2], uint32_t len[2], uint32_t* ranges);
/* reader().set_error() */
int ics_rx_stream_set_error(ics_rx_stream* rxs);

/* The copy kernel on its own (k_copy_pieces): for each of m pieces in device
 * memory, d_dst[dst .. dst + len) = d_src[src .. src + len).  Contract:
 * destinations pairwise disjoint; the two buffers do not overlap; every piece
 * inside src_bytes / dst_bytes; len may be 0; neither src nor dst (nor the
 * two bases) needs any alignment; dst_bytes <= 2^31.  Loads stay inside the
 * aligned 16-byte blocks that hold a piece's source bytes; a destination block
 * shared with a neighbouring piece is written with stores that cover only this
 * piece's bytes (never read, merged and written back).  m == 0 launches
 * nothing.  libicsum_debug.so checks every load against the piece's envelope
 * and the source buffer and every store against [0, dst_bytes). */
int ics_copy_pieces(ics_ctx* ctx, const void* d_src, uint64_t src_bytes, void* d_dst, uint64_t dst_bytes,
                    const ics_copy_piece* d_pieces, uint64_t m, void* stream);

/* The ring's device pointer (capacity bytes). */
int ics_rx_stream_ring(ics_rx_stream* rxs, void** d_ring);
/* One batch on the device: plans as ics_rx_stream_plan (the records, take and
 * the offsets are HOST arrays — the offsets the caller uploaded for
 * ics_tcp_unwrap_batch; d_dgrams is that call's device buffer), puts the copy
 * list where the device reads it and launches k_copy_pieces on `stream`;
 * nothing is launched when the list is empty.  The host state (send, stats,
 * peek) is final on return; the bytes are in the ring once `stream` reaches the
 * launch.  The copy list travels through a leased page-locked area that only
 * grows, its event recorded behind the launch: no allocation and no
 * synchronisation in the steady state.  Ordering is the caller's: calls on one
 * ics_rx_stream go on one stream, or are synchronised between streams.
 * The call plans on a copy of the state and commits it once the copy is
 * enqueued: after ANY error (argument, ICS_ERR_NOMEM, ICS_ERR_HIP) the stream
 * is as it was.  ICS_ERR_INVALID: a null context, stream or
 * (n > 0) records, a stream without a ring or of another context, and what
 * ics_rx_stream_plan refuses. */
int ics_rx_stream_receive_batch(ics_ctx* ctx, ics_rx_stream* rxs, const void* d_dgrams, const uint64_t* h_offsets,
                                uint64_t stride, uint64_t dgram_len, uint64_t n, const ics_tcp_rx* h_recs,
                                const uint8_t* h_take, void* stream);
/* read(): up to len buffered bytes to h_dst — peek, one or two copies on
 * `stream`, synchronise, pop.  *got = the bytes read. */
int ics_rx_stream_read(ics_ctx* ctx, ics_rx_stream* rxs, void* h_dst, uint64_t len, uint64_t* got, void* stream);

/* ---- several batches in one launch -------------------------------------- */
/* The receive and transmit paths hand the engine a stream of small batches —
 * one per event-loop tick or per filled arena (the reference reads its TUN fd
 * one datagram per call, util/tuntap/tuntap_adapter.cpp:5-21, inside the
 * socket's event loop, util/tcp_minnow_socket/tcp_minnow_socket.h:138-164).
 * Each launch pays a fixed ramp and drain of a few microseconds, so k such
 * batches queued together run as ONE launch per kernel shape (batches of up
 * to 16 per launch): results identical to k calls of ics_checksum_batch /
 * ics_ipv4_tcp_batch on the same arguments, in any order (the batches must
 * not overlap where PATCH writes).  Fixed-stride batches take the geometry
 * their length picks; offsets batches take the unplanned default (no
 * binning: call ics_checksum_batch for one large mixed batch).  The
 * descriptor arrays are host memory, read before the call returns. */
typedef struct ics_seg_batch {
  const void* bytes;         /* d_bytes of ics_checksum_batch */
  const uint64_t* offsets;   /* d_offsets (NULL: fixed stride) */
  uint64_t stride, seg_len, n;
  const uint32_t* init;      /* d_init (NULL = 0) */
  uint16_t* out;             /* d_out */
} ics_seg_batch;
int ics_checksum_batchv(ics_ctx* ctx, const ics_seg_batch* batches, uint32_t k, void* stream);

typedef struct ics_dgram_batch {
  void* dgrams;              /* d_dgrams of ics_ipv4_tcp_batch */
  const uint64_t* offsets;   /* d_offsets (NULL: fixed stride) */
  uint64_t stride, dgram_len, n;
  uint16_t* ip_ck;           /* each output may be NULL */
  uint16_t* tcp_ck;
  uint8_t* status;
} ics_dgram_batch;
int ics_ipv4_tcp_batchv(ics_ctx* ctx, const ics_dgram_batch* batches, uint32_t k, int mode, void* stream);

/* ---- host-memory variants (PCIe-inclusive path) ------------------------ */
/* Same semantics as ics_checksum_batch / ics_ipv4_tcp_batch on host
 * buffers; ics_checksum_batch_host takes segments of any length (longer than
 * a staging slot: summed piecewise, parity carried, as add() chains do).  The engine stages through pinned memory in chunks (page-locked
 * caller buffers are DMA'd directly) and pipelines H2D / kernel / D2H on its
 * slot streams; returns when the outputs are complete.  PATCH on host
 * memory: the device computes the two checksums and the engine writes the
 * two fields into h_dgrams on the host (same bytes as the device PATCH). */
int ics_checksum_batch_host(ics_ctx* ctx, const void* h_bytes, const uint64_t* h_offsets,
                            uint64_t stride, uint64_t seg_len, const uint32_t* h_init,
                            uint16_t* h_out, uint64_t n);
int ics_ipv4_tcp_batch_host(ics_ctx* ctx, void* h_dgrams, const uint64_t* h_offsets,
                            uint64_t stride, uint64_t dgram_len, uint64_t n, int mode,
                            uint16_t* h_ip_ck, uint16_t* h_tcp_ck, uint8_t* h_status);
/* ics_tcp_wrap_batch on host memory (e.g. a page-locked DatagramBatch arena
 * the payloads were copied into once): the payload bytes go to the device,
 * only the 40 header bytes per datagram come back and are written into
 * h_dgrams.  Synchronous. */
int ics_tcp_wrap_batch_host(ics_ctx* ctx, void* h_dgrams, const uint64_t* h_offsets, uint64_t stride,
                            uint64_t dgram_len, uint64_t n, const ics_tcp_msg* h_msgs);
/* ics_tcp_wrap_headers on host memory: payloads in, 40 header bytes per
 * datagram out into h_hdrs.  Synchronous. */
int ics_tcp_wrap_headers_host(ics_ctx* ctx, const void* h_payloads, const uint64_t* h_offsets, uint64_t stride,
                              uint64_t payload_len, uint64_t n, const ics_tcp_msg* h_msgs, void* h_hdrs);

/* Resident tick server (not a reference interface).  idle_us > 0: the
 * zero-copy *_host calls of at most 16 x blocks segments (checksum, fused
 * IPv4 in any mode, both wraps; fixed stride or offsets) are taken by a
 * kernel of `blocks` blocks that stays resident on the context's GPU between
 * calls and reads each call's job from mailboxes in page-locked memory (16
 * segments per block) — no kernel launch per call.  It leaves after idle_us
 * microseconds without a call (the next call launches it again) or on
 * ics_set_tick_server(ctx, 0) / ics_destroy.  While it is resident the
 * device is busy: hipDeviceSynchronize waits until it leaves.  Results are
 * identical to the launched path.  0 (default): off. */
int ics_set_tick_server(ics_ctx* ctx, uint32_t idle_us);
/* The server's blocks, 1..8 (default 4: ticks of up to 64 segments).  Each
 * resident block keeps one CU and one poll of its mailbox in flight over
 * PCIe; a tick of at most 16 segments costs the same with any number.
 * Takes effect at the server's next launch (a running server is stopped). */
int ics_set_tick_server_blocks(ics_ctx* ctx, uint32_t blocks);

/* ---- device memory helpers for FFI callers without an allocator -------- */
int ics_malloc(ics_ctx* ctx, void** d_ptr, size_t bytes);
int ics_free(ics_ctx* ctx, void* d_ptr);
/* Page-locked host memory: batches in it are DMA'd by the *_host calls with
 * no staging copy (the receive/transmit rings of a batched TUN/socket path). */
int ics_host_alloc(ics_ctx* ctx, void** h_ptr, size_t bytes);
int ics_host_free(ics_ctx* ctx, void* h_ptr);
int ics_memcpy_htod(ics_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, void* stream);
int ics_memcpy_dtoh(ics_ctx* ctx, void* h_dst, const void* d_src, size_t bytes, void* stream);
int ics_stream_synchronize(ics_ctx* ctx, void* stream);

/* ---- diagnostics (not a reference interface) ----------------------------- */
/* Which launch the last batch call on this context issued, and the plan
 * cache's counters since ics_create: a caller can check that its steady-state
 * batches hit the cached plan (and tests check which kernel ran).  Racy
 * snapshots when several threads share the context. */
#define ICS_K_CHECKSUM 1         /* k_checksum: one lane group per segment */
#define ICS_K_SMALL 2            /* k_checksum_small: several short segments per lane group */
#define ICS_K_TINY 3             /* k_checksum_tiny: one lane per segment */
#define ICS_K_DENSE 4            /* k_checksum_dense: fixed stride == length in {32, 64, 128} */
#define ICS_K_TWOCLASS 5         /* k_checksum_twoclass: short segments one per lane, long ones 16 lanes */
#define ICS_K_BINNED 6           /* the length-binning passes + bin launches */
#define ICS_K_IPV4 7             /* k_ipv4_tcp */
#define ICS_K_IPV4_TWOCLASS 8    /* k_ipv4_twoclass */
#define ICS_K_WRAP 9             /* k_tcp_wrap, one pass */
#define ICS_K_WRAP_2PASS 10      /* k_tcp_wrap (payload sums) + k_tcp_hdr */
#define ICS_K_ROUTER 11          /* k_router_ttl */
#define ICS_K_BATCHV 12          /* several batches in one launch (ics_*_batchv) */
#define ICS_K_TILE 13            /* k_span: an offsets batch as one packed stream, S (1..63) segments per wave */
#define ICS_K_ROUTER_HDRS 14     /* k_router_hdrs: the router step, forwarded headers apart */
#define ICS_K_TICK 15            /* k_tick: a zero-copy *_host tick of <= 16 offsets segments, offsets in the kernel arguments */
#define ICS_K_TICK_SERVER 16     /* the resident tick server took the tick (ics_set_tick_server) */
#define ICS_K_ROUTE_LOOKUP 17    /* k_route_lookup: one lane per address */
#define ICS_K_ROUTER_ROUTE 18    /* k_router_ttl with the route lookup fused */
#define ICS_K_ROUTER_ROUTE_HDRS 19 /* k_router_hdrs with the route lookup fused */
#define ICS_K_FRAME_RECV 20      /* k_frame<false>: recv_frame's classification (0 / 0) */
#define ICS_K_ROUTER_FRAMES 21   /* k_frame<true>: the whole hop over Ethernet frames (0 / 0) */
#define ICS_K_UNWRAP 22          /* k_tcp_unwrap behind the VERIFY launch: ics_tcp_unwrap_batch(_host) (0 / 0) */
#define ICS_K_COPY_PIECES 23     /* k_copy_pieces: ics_copy_pieces, ics_rx_stream_receive_batch (0 / 0) */
/* last_lps / last_unroll by kernel:
 *   ICS_K_CHECKSUM .. ICS_K_WRAP_2PASS  lanes per segment / loads in flight per lane
 *   ICS_K_TWOCLASS, ICS_K_IPV4_TWOCLASS  long-segment lanes (16) / segments per wave (16 or 32; 8 only under ICSUM_FORCE twoclass=8)
 *   ICS_K_BATCHV  the ICS_BV_* shape of the last launch group / batches in the call
 *   ICS_K_TILE    segments per wave S / ICS_TILE_* operation; S is chosen per
 *                 call, clamp(20 KiB / mean segment length, 1, 63) from the
 *                 cached plan (ICSUM_FORCE span_segs pins it)
 *   ICS_K_ROUTER, ICS_K_ROUTER_HDRS  0 / 0
 *   ICS_K_ROUTE_LOOKUP, ICS_K_ROUTER_ROUTE, ICS_K_ROUTER_ROUTE_HDRS  0 / 0
 *   ICS_K_TICK, ICS_K_TICK_SERVER  16 / 8 (a 16-lane group per segment, one block) */
#define ICS_BV_DENSE64 0 /* fixed stride == length == 64 B, 16-byte aligned */
#define ICS_BV_TINY 1    /* one lane per segment (ACK-sized fixed lengths) */
#define ICS_BV_SMALL 2   /* 4-lane groups, two segments in flight */
#define ICS_BV_LINE16 3  /* 16-lane line grid */
#define ICS_BV_LINE64 4  /* 64-lane line grid */
#define ICS_BV_LANE1 5   /* fused IPv4 kernel, one lane per ACK-sized datagram */
#define ICS_TILE_CHECKSUM 0
#define ICS_TILE_IPV4 1
#define ICS_TILE_WRAP 2
#define ICS_TILE_WRAP_APART 3
typedef struct ics_dispatch_info_t {
  uint64_t plan_hits;      /* lookups that found this batch's landed plan */
  uint64_t plan_misses;    /* lookups that did not (first call, plan still in flight) */
  uint64_t plan_requests;  /* plan kernels queued behind launches */
  int32_t last_kernel;     /* ICS_K_* of the last call's main launch (0: none yet) */
  int32_t last_lps;        /* its lanes per segment (other kernels: see the table above) */
  int32_t last_unroll;     /* its loads in flight per lane (other kernels: see the table above) */
  int32_t last_plan;       /* the cached plan it followed (k_bin_plan ids 0-3), -1 none */
  uint64_t host_zero_copy; /* *_host calls whose batch the kernel read in place (one chunk, no DMA) */
  uint64_t host_dma_chunks; /* staged chunks (and long-segment pieces) the *_host calls DMA'd */
} ics_dispatch_info_t;
int ics_dispatch_info(const ics_ctx* ctx, ics_dispatch_info_t* info);

#ifdef __cplusplus
}
#endif

#endif /* ICSUM_H */
