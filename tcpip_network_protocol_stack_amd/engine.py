"""Python host mirror of the checksum engine (plumbing over libicsum.so).

The reference's interface for this path is the C++ header surface of
util/tools/checksum.h, util/ipv4_header, util/tcp_segment and util/tcp_over_ip
(SURVEY.md §8b); its C++ mirror lives in csrc/host/.  This module exposes the
same batch entry points to Python for tests and bench.py.  Device memory and
streams come from PyTorch (plumbing only); every byte of arithmetic runs in
the HIP kernels behind the C-ABI.  There is no fallback: a missing library or
GPU raises.
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check

MODE_COMPUTE, MODE_VERIFY, MODE_PATCH = _lib.ICS_MODE_COMPUTE, _lib.ICS_MODE_VERIFY, _lib.ICS_MODE_PATCH
ST_ACCEPT = _lib.ICS_ST_ACCEPT
TCP_FIN, TCP_SYN, TCP_RST, TCP_ACK = _lib.ICS_TCP_FIN, _lib.ICS_TCP_SYN, _lib.ICS_TCP_RST, _lib.ICS_TCP_ACK

# struct ics_tcp_msg (include/icsum.h) as a numpy record
TCP_MSG_DTYPE = np.dtype([("src", "<u4"), ("dst", "<u4"), ("seqno", "<u4"), ("ackno", "<u4"),
                          ("src_port", "<u2"), ("dst_port", "<u2"), ("window", "<u2"), ("flags", "u1"),
                          ("ttl", "u1"), ("id", "<u2"), ("reserved", "<u2")])
assert TCP_MSG_DTYPE.itemsize == 28
# struct ics_tcp_rx (include/icsum.h) as a numpy record
TCP_RX_DTYPE = np.dtype([("msg", TCP_MSG_DTYPE), ("pay_off", "<u4"), ("pay_len", "<u4"), ("status", "u1"),
                         ("reserved", "u1", (3,))])
assert TCP_RX_DTYPE.itemsize == 40
# struct ics_copy_piece (include/icsum.h) as a numpy record
COPY_PIECE_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u4"), ("len", "<u4")])
assert COPY_PIECE_DTYPE.itemsize == 16


def _ptr(t):
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


def _stream(stream, device):
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)


def _count(n, offsets, data, stride):
    """Segments of a batch: n when given, else from the offsets (n + 1
    entries), else from a positive fixed stride; a fixed-stride batch with no
    stride and no n is an error (not one segment per byte)."""
    if n is not None:
        return int(n)
    if offsets is not None:
        return offsets.numel() - 1
    if not stride or stride <= 0:
        raise ValueError("batch without n, offsets or a positive stride")
    return data.numel() // stride


class RouteTable:
    """ics_route_table_*: a route table with Router::match's semantics
    (src/router/router.cpp:15-24, :77-87; include/icsum.h has the rules).
    Needs no Engine and no GPU.  debug=True: a table of libicsum_debug.so,
    for an Engine(debug=True) — a table belongs to the library that made it."""

    def __init__(self, debug=False):
        self.debug = bool(debug)
        self.lib = _lib.load(_lib.DEBUG_LIB_PATH if debug else None)
        h = ctypes.c_void_p()
        check(self.lib.ics_route_table_create(ctypes.byref(h)), self.lib)
        self.handle = h

    def add(self, prefix, prefix_len, iface, next_hop=None):
        """Router::add_route; next_hop None = a direct route (0 is a next hop
        of 0.0.0.0, not "direct")."""
        check(self.lib.ics_route_table_add(self.handle, prefix & 0xFFFFFFFF, prefix_len, iface,
                                           next_hop is not None, (next_hop or 0) & 0xFFFFFFFF), self.lib)

    def clear(self):
        check(self.lib.ics_route_table_clear(self.handle), self.lib)

    def match(self, addr):
        """(iface, next_hop.value_or(addr)) or None."""
        f, h = ctypes.c_uint32(), ctypes.c_uint32()
        rc = self.lib.ics_route_table_match(self.handle, addr & 0xFFFFFFFF, ctypes.byref(f), ctypes.byref(h))
        if rc < 0:
            check(rc, self.lib)
        return (f.value, h.value) if rc else None

    def stats(self):
        st = _lib.RouteStats()
        check(self.lib.ics_route_table_stats(self.handle, ctypes.byref(st)), self.lib)
        return {k: getattr(st, k) for k, _ in st._fields_}

    def close(self):
        if self.handle:
            self.lib.ics_route_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NeighTable:
    """ics_neigh_table_*: the control half of the router's NetworkInterfaces
    (src/network_interface/network_interface.cpp; include/icsum.h has the
    rules) — per-interface addresses, ARP cache and pending requests.  Needs
    no Engine and no GPU.  Addresses are 6-byte `bytes`, ips host-order ints.
    The queue of datagrams waiting for a reply is the caller's.  debug=True: a
    table of libicsum_debug.so, for an Engine(debug=True)."""

    def __init__(self, debug=False):
        self.debug = bool(debug)
        self.lib = _lib.load(_lib.DEBUG_LIB_PATH if debug else None)
        h = ctypes.c_void_p()
        check(self.lib.ics_neigh_table_create(ctypes.byref(h)), self.lib)
        self.handle = h

    def set_iface(self, iface, mac, ip):
        """NetworkInterface's constructor: interface `iface` has these addresses."""
        check(self.lib.ics_neigh_table_set_iface(self.handle, iface, bytes(mac), ip & 0xFFFFFFFF), self.lib)

    def learn(self, iface, ip, mac):
        check(self.lib.ics_neigh_table_learn(self.handle, iface, ip & 0xFFFFFFFF, bytes(mac)), self.lib)

    def lookup(self, iface, ip):
        """the neighbour's address (bytes) or None; walks the compiled image"""
        mac = ctypes.create_string_buffer(6)
        rc = self.lib.ics_neigh_table_lookup(self.handle, iface, ip & 0xFFFFFFFF, mac)
        if rc < 0:
            check(rc, self.lib)
        return mac.raw if rc else None

    def tick(self, ms, iface=_lib.ICS_ALL_IFACES):
        check(self.lib.ics_neigh_table_tick(self.handle, iface, int(ms)), self.lib)

    def recv_frame(self, iface, frame):
        """recv_frame for one frame: (status, events, sender_ip, reply) — reply
        is the 42-byte ARP reply to transmit when events has ICS_ARP_REPLY,
        else None."""
        frame = bytes(frame)
        st, ev, sip = ctypes.c_uint8(), ctypes.c_uint32(), ctypes.c_uint32()
        reply = ctypes.create_string_buffer(42)
        check(self.lib.ics_neigh_table_recv_frame(self.handle, iface, frame, len(frame), ctypes.byref(st),
                                                  ctypes.byref(ev), ctypes.byref(sip), reply), self.lib)
        return st.value, ev.value, sip.value, reply.raw if ev.value & _lib.ICS_ARP_REPLY else None

    def resolve(self, iface, next_hop):
        """send_datagram's control half: (hdr14, None) on a hit, else (None,
        request) with the 42-byte ARP request to transmit, or (None, None)
        while one is pending (or the interface has no addresses)."""
        hdr, req, ev = ctypes.create_string_buffer(14), ctypes.create_string_buffer(42), ctypes.c_uint32()
        rc = self.lib.ics_neigh_table_resolve(self.handle, iface, next_hop & 0xFFFFFFFF, hdr, ctypes.byref(ev), req)
        if rc < 0:
            check(rc, self.lib)
        if rc:
            return hdr.raw, None
        return None, req.raw if ev.value & _lib.ICS_ARP_REQUEST else None

    def stats(self):
        st = _lib.NeighStats()
        check(self.lib.ics_neigh_table_stats(self.handle, ctypes.byref(st)), self.lib)
        return {k: getattr(st, k) for k, _ in st._fields_}

    def close(self):
        if self.handle:
            self.lib.ics_neigh_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RxStream:
    """ics_rx_stream_*: one connection's receive stream — TCPReceiver +
    Reassembler + the writer half of ByteStream on ics_tcp_rx records
    (include/icsum.h has the rules).  RxStream(capacity) is the CPU-only
    object (plan, send, stats, peek, pop: no Engine, no GPU);
    Engine.rx_stream(capacity) adds the ring in device memory and receive /
    read.  Records are TCP_RX_DTYPE arrays on the host."""

    def __init__(self, capacity, engine=None, debug=False):
        self.engine = engine
        self.lib = engine.lib if engine is not None else _lib.load(_lib.DEBUG_LIB_PATH if debug else None)
        h = ctypes.c_void_p()
        if engine is not None:
            check(self.lib.ics_rx_stream_create(engine.ctx, int(capacity), ctypes.byref(h)), self.lib)
        else:
            check(self.lib.ics_rx_stream_create_host(int(capacity), ctypes.byref(h)), self.lib)
        self.handle = h
        self.capacity = int(capacity)
        if engine is not None:  # a stream with a ring must go before its context: Engine.close() closes it
            engine._streams.add(self)

    @staticmethod
    def _batch(recs, take, offsets):
        recs = np.ascontiguousarray(recs, dtype=TCP_RX_DTYPE)
        take = None if take is None else np.ascontiguousarray(take, dtype=np.uint8)
        offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        return recs, take, offsets

    def plan(self, recs, take=None, offsets=None, stride=0, dgram_len=0, dry=False):
        """ics_rx_stream_plan over the records in order: the batch's copy list,
        a COPY_PIECE_DTYPE array (src: byte offset in the datagram buffer, dst:
        ring offset).  dry=True only counts (state unchanged) and returns m."""
        recs, take, offsets = self._batch(recs, take, offsets)
        m = ctypes.c_uint64()
        args = (self.handle, _ptr(recs), len(recs), _ptr(take), _ptr(offsets), stride, dgram_len)
        check(self.lib.ics_rx_stream_plan(*args, None, 0, ctypes.byref(m)), self.lib)
        if dry:
            return m.value
        pieces = np.empty(m.value, dtype=COPY_PIECE_DTYPE)
        check(self.lib.ics_rx_stream_plan(*args, pieces.ctypes.data, len(pieces), ctypes.byref(m)), self.lib)
        return pieces[:m.value]

    def receive(self, dgrams, recs, take=None, offsets=None, stride=0, dgram_len=0, stream=None):
        """ics_rx_stream_receive_batch: `dgrams` the device tensor the records
        were unwrapped from, `recs` / `take` / `offsets` host arrays.  The host
        state is final on return; the bytes follow on `stream`."""
        recs, take, offsets = self._batch(recs, take, offsets)
        e = self.engine
        check(self.lib.ics_rx_stream_receive_batch(e.ctx, self.handle, _ptr(dgrams), _ptr(offsets), stride, dgram_len,
                                                   len(recs), _ptr(recs), _ptr(take), _stream(stream, e.device)),
              self.lib)

    def send(self):
        """TCPReceiver::send: {'ackno' (None without an ISN), 'window', 'rst'}."""
        o = _lib.RxSend()
        check(self.lib.ics_rx_stream_send(self.handle, ctypes.byref(o)), self.lib)
        return {"ackno": o.ackno if o.has_ackno else None, "window": o.window, "rst": bool(o.rst)}

    def stats(self):
        st = _lib.RxStats()
        check(self.lib.ics_rx_stream_stats(self.handle, ctypes.byref(st)), self.lib)
        return {k: getattr(st, k) for k, _ in st._fields_}

    def peek(self):
        """[(ring offset, length), ...]: the 0, 1 or 2 ring ranges holding [popped, pushed)."""
        off, ln, k = (ctypes.c_uint32 * 2)(), (ctypes.c_uint32 * 2)(), ctypes.c_uint32()
        check(self.lib.ics_rx_stream_peek(self.handle, off, ln, ctypes.byref(k)), self.lib)
        return [(off[i], ln[i]) for i in range(k.value)]

    def pop(self, n):
        check(self.lib.ics_rx_stream_pop(self.handle, int(n)), self.lib)

    def set_error(self):
        check(self.lib.ics_rx_stream_set_error(self.handle), self.lib)

    def ring(self):
        """The ring's device address (ics_rx_stream_ring)."""
        p = ctypes.c_void_p()
        check(self.lib.ics_rx_stream_ring(self.handle, ctypes.byref(p)), self.lib)
        return p.value

    def read(self, n, stream=None):
        """ics_rx_stream_read: up to n buffered bytes (popped) as `bytes`."""
        buf = np.empty(max(int(n), 1), dtype=np.uint8)
        got = ctypes.c_uint64()
        e = self.engine
        check(self.lib.ics_rx_stream_read(e.ctx, self.handle, buf.ctypes.data, int(n), ctypes.byref(got),
                                          _stream(stream, e.device)), self.lib)
        return buf[:got.value].tobytes()

    def close(self):
        if self.handle:
            self.lib.ics_rx_stream_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One engine context bound to one GPU (ics_create / ics_destroy)."""

    def __init__(self, device=0, debug=False):
        """debug=True: the bounds-checked build (libicsum_debug.so)."""
        self.lib = _lib.load(_lib.DEBUG_LIB_PATH if debug else None)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        ctx = ctypes.c_void_p()
        self._check(self.lib.ics_create(self.device.index or 0, ctypes.byref(ctx)))
        self.ctx = ctx
        self._streams = weakref.WeakSet()  # rx_stream() objects, closed before the context

    def _check(self, rc):
        return check(rc, self.lib)

    def set_binning(self, mode):
        """Dispatch of offsets batches: _lib.ICS_BINNING_AUTO / SINGLE / BINNED
        (ics_set_binning)."""
        self._check(self.lib.ics_set_binning(self.ctx, int(mode)))

    def set_tick_server(self, idle_us):
        """ics_set_tick_server: idle_us > 0 keeps a resident kernel that takes
        the zero-copy *_host calls of <= 16 x blocks segments without a launch
        (it leaves after idle_us without a call); 0 stops it."""
        self._check(self.lib.ics_set_tick_server(self.ctx, int(idle_us)))

    def set_tick_server_blocks(self, blocks):
        """ics_set_tick_server_blocks: the resident server's blocks, 1..8
        (default 4), 16 segments per block."""
        self._check(self.lib.ics_set_tick_server_blocks(self.ctx, int(blocks)))

    def dispatch_info(self):
        """ics_dispatch_info: {'plan_hits', 'plan_misses', 'plan_requests',
        'kernel' (name of the last call's main launch), 'lps', 'unroll', 'plan',
        'host_zero_copy', 'host_dma_chunks' (the *_host pipeline's counters)}."""
        d = _lib.DispatchInfo()
        self._check(self.lib.ics_dispatch_info(self.ctx, ctypes.byref(d)))
        return {"plan_hits": d.plan_hits, "plan_misses": d.plan_misses, "plan_requests": d.plan_requests,
                "kernel": _lib.KERNELS.get(d.last_kernel), "lps": d.last_lps, "unroll": d.last_unroll,
                "plan": d.last_plan, "host_zero_copy": d.host_zero_copy, "host_dma_chunks": d.host_dma_chunks}

    def close(self):
        if self.ctx:
            for rx in list(self._streams):
                rx.close()
            self.lib.ics_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- a1-a4 -----------------------------------------------------------
    def checksum_batch(self, data, n=None, offsets=None, stride=0, seg_len=0, init=None, out=None,
                       stream=None):
        """u16 InternetChecksum{init_i}.add(segment_i).value() for every segment."""
        n = _count(n, offsets, data, stride)
        if out is None:
            out = torch.empty(n, dtype=torch.int16, device=self.device)
        self._check(self.lib.ics_checksum_batch(self.ctx, _ptr(data), _ptr(offsets), stride, seg_len,
                                          _ptr(init), _ptr(out), n, _stream(stream, self.device)))
        return out

    def sum_batch(self, data, n=None, offsets=None, stride=0, seg_len=0, init=None, odd=None,
                  out=None, stream=None):
        """Unfolded uint32 sum_ after add(segment_i) with parity odd_i (add() chains)."""
        n = _count(n, offsets, data, stride)
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self.lib.ics_sum_batch(self.ctx, _ptr(data), _ptr(offsets), stride, seg_len, _ptr(init),
                                     _ptr(odd), _ptr(out), n, _stream(stream, self.device)))
        return out

    def fold_batch(self, sums, out=None, stream=None):
        n = sums.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.int16, device=self.device)
        self._check(self.lib.ics_fold_batch(self.ctx, _ptr(sums), _ptr(out), n, _stream(stream, self.device)))
        return out

    def checksum_batchv(self, batches, stream=None):
        """ics_checksum_batchv: several checksum batches in one launch per
        kernel shape.  `batches`: dicts with keys data, n, offsets, stride,
        seg_len, init, out (out allocated when absent); returns the outs."""
        arr = (_lib.SegBatch * max(1, len(batches)))()
        outs = []
        for j, b in enumerate(batches):
            offsets = b.get("offsets")
            n = _count(b.get("n"), offsets, b["data"], b.get("stride", 0))
            out = b.get("out")
            if out is None:
                out = torch.empty(n, dtype=torch.int16, device=self.device)
            arr[j] = _lib.SegBatch(_ptr(b["data"]), _ptr(offsets), b.get("stride", 0), b.get("seg_len", 0), n,
                                   _ptr(b.get("init")), _ptr(out))
            outs.append(out)
        self._check(self.lib.ics_checksum_batchv(self.ctx, arr, len(batches), _stream(stream, self.device)))
        return outs

    def ipv4_tcp_batchv(self, batches, mode, stream=None):
        """ics_ipv4_tcp_batchv: dicts with keys dgrams, n, offsets, stride,
        dgram_len, ip_ck, tcp_ck, status (outputs allocated when absent);
        returns [(ip_ck, tcp_ck, status), ...]."""
        arr = (_lib.DgramBatch * max(1, len(batches)))()
        outs = []
        for j, b in enumerate(batches):
            offsets = b.get("offsets")
            n = _count(b.get("n"), offsets, b["dgrams"], b.get("stride", 0))
            mk = lambda dt: torch.empty(n, dtype=dt, device=self.device)  # noqa: E731
            o = tuple(b.get(k) if b.get(k) is not None else mk(dt)
                      for k, dt in (("ip_ck", torch.int16), ("tcp_ck", torch.int16), ("status", torch.uint8)))
            arr[j] = _lib.DgramBatch(_ptr(b["dgrams"]), _ptr(offsets), b.get("stride", 0), b.get("dgram_len", 0), n,
                                     _ptr(o[0]), _ptr(o[1]), _ptr(o[2]))
            outs.append(o)
        self._check(self.lib.ics_ipv4_tcp_batchv(self.ctx, arr, len(batches), mode, _stream(stream, self.device)))
        return outs

    # ---- fused IPv4 + TCP --------------------------------------------------
    def ipv4_tcp_batch(self, dgrams, mode, n=None, offsets=None, stride=0, dgram_len=0,
                       ip_ck=None, tcp_ck=None, status=None, stream=None):
        n = _count(n, offsets, dgrams, stride)
        mk = lambda dt: torch.empty(n, dtype=dt, device=self.device)  # noqa: E731
        ip_ck = mk(torch.int16) if ip_ck is None else ip_ck
        tcp_ck = mk(torch.int16) if tcp_ck is None else tcp_ck
        status = mk(torch.uint8) if status is None else status
        self._check(self.lib.ics_ipv4_tcp_batch(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len, n,
                                          mode, _ptr(ip_ck), _ptr(tcp_ck), _ptr(status),
                                          _stream(stream, self.device)))
        return ip_ck, tcp_ck, status

    # ---- device-side wrap (wrap_tcp_in_ip, tcp_over_ip.cpp:69-88) ----------
    def tcp_wrap_batch(self, dgrams, msgs, n=None, offsets=None, stride=0, dgram_len=0, ip_ck=None,
                       tcp_ck=None, stream=None):
        """Headers + both checksums of every datagram written in place on the
        device; `msgs` is a device tensor holding n ics_tcp_msg records."""
        n = _count(n, offsets, dgrams, stride)
        self._check(self.lib.ics_tcp_wrap_batch(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len, n,
                                          _ptr(msgs), _ptr(ip_ck), _ptr(tcp_ck), _stream(stream, self.device)))
        return dgrams

    def tcp_wrap_headers(self, payloads, msgs, hdrs, n=None, offsets=None, stride=0, payload_len=0, ip_ck=None,
                         tcp_ck=None, stream=None):
        """Payload-only batch; the 40 header bytes of datagram i go to hdrs[40 i:]."""
        n = _count(n, offsets, payloads, stride)
        self._check(self.lib.ics_tcp_wrap_headers(self.ctx, _ptr(payloads), _ptr(offsets), stride, payload_len, n,
                                                  _ptr(msgs), _ptr(hdrs), _ptr(ip_ck), _ptr(tcp_ck),
                                                  _stream(stream, self.device)))
        return hdrs

    def tcp_wrap_headers_host(self, payloads, msgs, n, offsets=None, stride=0, payload_len=0, hdrs=None):
        """Payload-only batch in host memory; the 40 header bytes of datagram i
        go to hdrs[40 i:] (a numpy uint8 array, allocated when absent)."""
        msgs = np.ascontiguousarray(msgs, dtype=TCP_MSG_DTYPE)
        hdrs = np.empty(n * 40, dtype=np.uint8) if hdrs is None else hdrs
        self._check(self.lib.ics_tcp_wrap_headers_host(self.ctx, _ptr(payloads), _ptr(offsets), stride, payload_len,
                                                       n, msgs.ctypes.data, hdrs.ctypes.data))
        return hdrs

    def tcp_wrap_batch_host(self, dgrams, msgs, n, offsets=None, stride=0, dgram_len=0):
        """The same on host memory (numpy uint8 datagrams, TCP_MSG_DTYPE records)."""
        msgs = np.ascontiguousarray(msgs, dtype=TCP_MSG_DTYPE)
        self._check(self.lib.ics_tcp_wrap_batch_host(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len, n,
                                               msgs.ctypes.data))
        return dgrams

    # ---- device-side unwrap (unwrap_tcp_in_ip, tcp_over_ip.cpp:14-64) -------
    def tcp_unwrap_batch(self, dgrams, n=None, offsets=None, stride=0, dgram_len=0, recs=None, status=None,
                         stream=None):
        """One 40-byte ics_tcp_rx per datagram (include/icsum.h has the rules):
        the VERIFY launch, then k_tcp_unwrap on the same stream.  `recs`: a
        uint8 device tensor of 40 n bytes, 4-byte aligned (allocated when
        absent); `status` (optional, n uint8) also receives the VERIFY status
        bytes.  Returns recs; view it with TCP_RX_DTYPE on the host."""
        n = _count(n, offsets, dgrams, stride)
        recs = torch.empty(n * 40, dtype=torch.uint8, device=self.device) if recs is None else recs
        self._check(self.lib.ics_tcp_unwrap_batch(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len, n,
                                                  _ptr(recs), _ptr(status), _stream(stream, self.device)))
        return recs

    # ---- receive streams (TCPReceiver + Reassembler per batch) --------------
    def rx_stream(self, capacity):
        """ics_rx_stream_create: a receive stream with its ring on this GPU."""
        return RxStream(capacity, engine=self)

    def copy_pieces(self, src, dst, pieces, m=None, stream=None):
        """ics_copy_pieces: dst[p.dst .. + p.len) = src[p.src .. + p.len) for
        the m ics_copy_piece records of the device tensor `pieces` (uint8,
        8-byte aligned); src / dst uint8 device tensors."""
        m = pieces.numel() // 16 if m is None else int(m)
        self._check(self.lib.ics_copy_pieces(self.ctx, _ptr(src), src.numel(), _ptr(dst), dst.numel(), _ptr(pieces),
                                             m, _stream(stream, self.device)))
        return dst

    def tcp_unwrap_batch_host(self, dgrams, n, offsets=None, stride=0, dgram_len=0, recs=None):
        """The same on host memory (numpy uint8 datagrams); returns a
        TCP_RX_DTYPE array of n records (`recs` when given)."""
        recs = np.empty(n, dtype=TCP_RX_DTYPE) if recs is None else recs
        self._check(self.lib.ics_tcp_unwrap_batch_host(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len, n,
                                                       _ptr(recs)))
        return recs

    def router_ttl_batch(self, dgrams, n=None, offsets=None, stride=0, dgram_len=0, status=None,
                         stream=None):
        n = _count(n, offsets, dgrams, stride)
        status = torch.empty(n, dtype=torch.uint8, device=self.device) if status is None else status
        self._check(self.lib.ics_router_ttl_batch(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len, n,
                                            _ptr(status), _stream(stream, self.device)))
        return status

    def router_ttl_headers(self, dgrams, n=None, offsets=None, stride=0, dgram_len=0, hdrs=None, status=None,
                           stream=None):
        """The router step with the forwarded 20-byte headers into `hdrs`
        (allocated when absent); the datagrams are only read.  Returns
        (hdrs, status)."""
        n = _count(n, offsets, dgrams, stride)
        hdrs = torch.empty(n * 20, dtype=torch.uint8, device=self.device) if hdrs is None else hdrs
        status = torch.empty(n, dtype=torch.uint8, device=self.device) if status is None else status
        self._check(self.lib.ics_router_ttl_headers(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len, n,
                                                    _ptr(hdrs), _ptr(status), _stream(stream, self.device)))
        return hdrs, status

    # ---- Router::match on the device ---------------------------------------
    def _table(self, table):
        if table.lib is not self.lib:
            raise ValueError("the route table belongs to the other library build (RouteTable(debug=...))")
        return table.handle

    def route_lookup_batch(self, table, addrs, n=None, iface=None, next_hop=None, stream=None):
        """match(addrs[i]) for a device tensor of host-order uint32 addresses
        (int32 storage); returns (iface, next_hop) int32 tensors, 0xFFFFFFFF /
        0 where no route matches."""
        n = addrs.numel() if n is None else int(n)
        iface = torch.empty(n, dtype=torch.int32, device=self.device) if iface is None else iface
        next_hop = torch.empty(n, dtype=torch.int32, device=self.device) if next_hop is None else next_hop
        self._check(self.lib.ics_route_lookup_batch(self.ctx, self._table(table), _ptr(addrs), n, _ptr(iface),
                                                    _ptr(next_hop), _stream(stream, self.device)))
        return iface, next_hop

    def router_route_batch(self, table, dgrams, n=None, offsets=None, stride=0, dgram_len=0, status=None,
                           iface=None, next_hop=None, stream=None):
        """Router::route in place: router_ttl_batch's step, then match(dst) of
        every datagram that forwards.  Returns (status, iface, next_hop);
        status bit 0 = forwarded, bit 1 = routed."""
        n = _count(n, offsets, dgrams, stride)
        status = torch.empty(n, dtype=torch.uint8, device=self.device) if status is None else status
        iface = torch.empty(n, dtype=torch.int32, device=self.device) if iface is None else iface
        next_hop = torch.empty(n, dtype=torch.int32, device=self.device) if next_hop is None else next_hop
        self._check(self.lib.ics_router_route_batch(self.ctx, self._table(table), _ptr(dgrams), _ptr(offsets), stride,
                                                    dgram_len, n, _ptr(status), _ptr(iface), _ptr(next_hop),
                                                    _stream(stream, self.device)))
        return status, iface, next_hop

    def router_route_headers(self, table, dgrams, n=None, offsets=None, stride=0, dgram_len=0, hdrs=None,
                             status=None, iface=None, next_hop=None, stream=None):
        """The same with the forwarded 20-byte headers into `hdrs` (as
        router_ttl_headers); returns (hdrs, status, iface, next_hop)."""
        n = _count(n, offsets, dgrams, stride)
        hdrs = torch.empty(n * 20, dtype=torch.uint8, device=self.device) if hdrs is None else hdrs
        status = torch.empty(n, dtype=torch.uint8, device=self.device) if status is None else status
        iface = torch.empty(n, dtype=torch.int32, device=self.device) if iface is None else iface
        next_hop = torch.empty(n, dtype=torch.int32, device=self.device) if next_hop is None else next_hop
        self._check(self.lib.ics_router_route_headers(self.ctx, self._table(table), _ptr(dgrams), _ptr(offsets),
                                                      stride, dgram_len, n, _ptr(hdrs), _ptr(status), _ptr(iface),
                                                      _ptr(next_hop), _stream(stream, self.device)))
        return hdrs, status, iface, next_hop

    # ---- Ethernet frames through the hop -----------------------------------
    def _neigh(self, table):
        if table.lib is not self.lib:
            raise ValueError("the neighbour table belongs to the other library build (NeighTable(debug=...))")
        return table.handle

    def frame_recv(self, neigh, frames, n=None, offsets=None, stride=0, frame_len=0, in_iface=0, in_ifaces=None,
                   status=None, stream=None):
        """recv_frame's classification of n Ethernet frames that arrived on
        in_iface (or in_ifaces[i], an int32 device tensor): the ICS_FR_* bits
        per frame.  The frames are only read."""
        n = _count(n, offsets, frames, stride)
        status = torch.empty(n, dtype=torch.uint8, device=self.device) if status is None else status
        self._check(self.lib.ics_frame_recv_batch(self.ctx, self._neigh(neigh), _ptr(frames), _ptr(offsets), stride,
                                                  frame_len, n, in_iface, _ptr(in_ifaces), _ptr(status),
                                                  _stream(stream, self.device)))
        return status

    def router_frames(self, routes, neigh, frames, n=None, offsets=None, stride=0, frame_len=0, in_iface=0,
                      in_ifaces=None, hdrs=None, status=None, iface=None, next_hop=None, stream=None):
        """The whole hop: classification, Router::route on the datagram at
        frame + 14, and the neighbour lookup on the egress interface, against
        the neighbour table as of the call.  Returns (hdrs, status, iface,
        next_hop); hdrs holds one 36-byte record per frame (2 zero bytes, the
        Ethernet header, the 20 forwarded header bytes)."""
        n = _count(n, offsets, frames, stride)
        hdrs = torch.empty(n * 36, dtype=torch.uint8, device=self.device) if hdrs is None else hdrs
        status = torch.empty(n, dtype=torch.uint8, device=self.device) if status is None else status
        iface = torch.empty(n, dtype=torch.int32, device=self.device) if iface is None else iface
        next_hop = torch.empty(n, dtype=torch.int32, device=self.device) if next_hop is None else next_hop
        self._check(self.lib.ics_router_frames(self.ctx, self._table(routes), self._neigh(neigh), _ptr(frames),
                                               _ptr(offsets), stride, frame_len, n, in_iface, _ptr(in_ifaces),
                                               _ptr(hdrs), _ptr(status), _ptr(iface), _ptr(next_hop),
                                               _stream(stream, self.device)))
        return hdrs, status, iface, next_hop

    # ---- host-memory (PCIe-inclusive) variants -----------------------------
    def checksum_batch_host(self, data, n, offsets=None, stride=0, seg_len=0, init=None, out=None):
        """Host-memory outputs (numpy, at least n elements) are allocated when absent."""
        out = np.empty(n, dtype=np.uint16) if out is None else out
        self._check(self.lib.ics_checksum_batch_host(self.ctx, _ptr(data), _ptr(offsets), stride, seg_len,
                                               _ptr(init), _ptr(out), n))
        return out

    def ipv4_tcp_batch_host(self, dgrams, n, mode, offsets=None, stride=0, dgram_len=0, ip_ck=None, tcp_ck=None,
                            status=None):
        ip = np.empty(n, dtype=np.uint16) if ip_ck is None else ip_ck
        tcp = np.empty(n, dtype=np.uint16) if tcp_ck is None else tcp_ck
        st = np.empty(n, dtype=np.uint8) if status is None else status
        self._check(self.lib.ics_ipv4_tcp_batch_host(self.ctx, _ptr(dgrams), _ptr(offsets), stride, dgram_len,
                                               n, mode, _ptr(ip), _ptr(tcp), _ptr(st)))
        return ip, tcp, st

    # ---- synthetic workloads (include/icsum_workload.h) -------------------
    def fill_bytes(self, t, seed, pos0=0, stream=None):
        self._check(self.lib.icsw_fill_bytes(self.ctx, _ptr(t), t.numel() * t.element_size(), seed, pos0,
                                       _stream(stream, self.device)))
        return t

    def pseudo_inits(self, n, seed, offsets=None, seg_len=0, index0=0, out=None, stream=None):
        out = torch.empty(n, dtype=torch.int32, device=self.device) if out is None else out
        self._check(self.lib.icsw_pseudo_inits(self.ctx, _ptr(out), _ptr(offsets), seg_len, n, seed, index0,
                                         _stream(stream, self.device)))
        return out

    def ipv4_tcp_headers(self, dgrams, n, stride, dgram_len, seed, index0=0, stream=None):
        self._check(self.lib.icsw_ipv4_tcp_headers(self.ctx, _ptr(dgrams), stride, dgram_len, n, seed, index0,
                                             _stream(stream, self.device)))
        return dgrams


def device_count():
    c = ctypes.c_int()
    check(_lib.load().ics_device_count(ctypes.byref(c)))
    return c.value


def tcp_unwrap_one(dgram, lib=None):
    """ics_tcp_unwrap_one: the record of one datagram (bytes), computed on the
    host with no context and no GPU; a _lib.TcpRx.  `lib`: a loaded library
    (default libicsum.so)."""
    lib = lib or _lib.load()
    dgram = bytes(dgram)
    rec = _lib.TcpRx()
    check(lib.ics_tcp_unwrap_one(dgram, len(dgram), ctypes.byref(rec)), lib)
    return rec


def mixed_offsets(n, seed):
    """Packed uint64 offsets (n+1) of the mixed-length workload (host)."""
    off = np.empty(n + 1, dtype=np.uint64)
    check(_lib.load().icsw_mixed_offsets(off.ctypes.data, n, seed))
    return off


def as_u16(t):
    return t.cpu().numpy().view(np.uint16)


def as_u32(t):
    return t.cpu().numpy().view(np.uint32)
