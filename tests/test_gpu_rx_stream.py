"""GPU tests of the receive streams: k_copy_pieces through ics_copy_pieces
against numpy, and ics_rx_stream_receive_batch / ics_rx_stream_read end to end
on wire datagrams — the release library and libicsum_debug.so, whose kernel
checks every source block against the piece's envelope and the source buffer
and every store against the ring.  The inventory entry is README_reasm.md."""
import random
import threading

import numpy as np
import pytest

from conftest import engine_with
from reasm_ref import RefStream
from rx_driver import (ISNS, batches, flags_of, lib_answers, load_golden, payload_of, random_stream, ref_apply,
                       run_scenario)
from unwrap_ref import wrap40

pytestmark = pytest.mark.gpu

SENT = 0xA5


@pytest.fixture(scope="module", params=[False, True], ids=["release", "debug"])
def reng(request):
    gen = engine_with(None, debug=request.param)
    yield next(gen)
    next(gen, None)


def _torch():
    import torch

    return torch


def _dev(a):
    return _torch().from_numpy(np.array(a, copy=True)).cuda()


def _pieces(src, dst, ln):
    from tcpip_network_protocol_stack_amd.engine import COPY_PIECE_DTYPE

    p = np.zeros(len(src), COPY_PIECE_DTYPE)
    p["src"], p["dst"], p["len"] = src, dst, ln
    return p


def copy_check(eng, src_np, dst_bytes, pieces, tag, lead=(0, 0)):
    """ics_copy_pieces on the device against numpy: the destination equal byte
    for byte (sentinels between and around the pieces intact), the source
    untouched, the dispatch id"""
    torch = _torch()
    ls, ld = lead  # byte bases at +ls / +ld inside their tensors
    src = _dev(np.concatenate([np.full(ls, 0x11, np.uint8), src_np]))
    dst = torch.full((ld + dst_bytes,), SENT, dtype=torch.uint8, device="cuda:0")
    dp = _dev(pieces.view(np.uint8)) if len(pieces) else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
    eng.copy_pieces(src[ls:], dst[ld:], dp, m=len(pieces))
    want = np.full(dst_bytes, SENT, np.uint8)
    for p in pieces:
        want[p["dst"]:p["dst"] + p["len"]] = src_np[p["src"]:p["src"] + p["len"]]
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got[ld:] != want)
    assert bad.size == 0, (tag, bad[:8].tolist(), got[ld:][bad[:8]].tolist(), want[bad[:8]].tolist())
    assert (got[:ld] == SENT).all(), tag
    assert (src.cpu().numpy()[ls:] == src_np).all(), tag
    if len(pieces):
        assert eng.dispatch_info()["kernel"] == "copy_pieces", tag


def _packed(lens, sres, dres):
    """pieces laid one behind the other, piece k's source at residue sres[k]
    and its destination at residue dres[k] mod 16: neighbours share blocks on
    both sides, with gaps of fewer than 16 sentinel bytes between them"""
    src, dst, s, d = [], [], 0, 0
    for n, a, b in zip(lens, sres, dres):
        s += (a - s) % 16
        d += (b - d) % 16
        src.append(s)
        dst.append(d)
        s += n
        d += n
    return np.array(src), np.array(dst), s, d


def test_every_length_and_residue_pair(reng):
    lens, sres, dres = np.meshgrid(np.arange(81), np.arange(16), np.arange(16), indexing="ij")
    order = np.random.default_rng(1).permutation(lens.size)
    lens, sres, dres = lens.ravel()[order], sres.ravel()[order], dres.ravel()[order]
    assert lens.size == 20736
    src, dst, ns, nd = _packed(lens, sres, dres)
    data = np.random.default_rng(2).integers(0, 256, ns, dtype=np.uint8)
    for lead in ((0, 0), (3, 0), (0, 5), (7, 9)):  # the byte bases off the 16-byte grid too
        copy_check(reng, data, nd, _pieces(src, dst, lens), ("lattice", lead), lead)


@pytest.mark.parametrize("n", [255, 256, 257, 1459, 1460, 1461, 4095, 4096, 4097, 65495])
def test_long_pieces(reng, n):
    pairs = [(0, 0), (1, 15), (13, 2), (7, 7)]
    src, dst, ns, nd = _packed([n] * 4, [a for a, _ in pairs], [b for _, b in pairs])
    data = np.random.default_rng(n).integers(0, 256, ns, dtype=np.uint8)
    copy_check(reng, data, nd, _pieces(src, dst, [n] * 4), ("long", n))


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 2051])
def test_piece_counts(reng, m):
    rng = np.random.default_rng(m)
    lens = rng.choice([0, 1, 5, 16, 17, 40, 100, 1460], m)
    src, dst, ns, nd = _packed(lens, rng.integers(0, 16, m), rng.integers(0, 16, m))
    data = rng.integers(0, 256, max(ns, 1), dtype=np.uint8)
    before = reng.dispatch_info()
    copy_check(reng, data, max(nd, 1), _pieces(src, dst, lens), ("count", m))
    if m == 0:
        assert reng.dispatch_info() == before  # nothing launched


def test_pieces_ending_at_the_allocations_last_byte(reng):
    """the aligned block behind the last source byte / ring byte reaches past
    the tensor: the load is clamped to the piece's blocks, the store narrow"""
    rng = np.random.default_rng(9)
    for ns, nd, n in ((1000 + 5, 777, 37), (4099, 2048 + 3, 300), (21, 13, 13), (33, 1, 1)):
        data = rng.integers(0, 256, ns, dtype=np.uint8)
        # one piece whose source ends the source, one whose destination ends the ring
        p = _pieces([ns - n, 1], [0, nd - n], [n, n]) if nd >= 2 * n else _pieces([ns - n], [nd - n], [n])
        copy_check(reng, data, nd, p, ("last byte", ns, nd, n))


def test_sources_on_both_sides_of_4gib(reng):
    torch = _torch()
    B32 = 1 << 32
    big = torch.empty(B32 + (1 << 20), dtype=torch.uint8, device="cuda:0")
    rng = np.random.default_rng(32)
    spots = [B32 - 70000, B32 - 1461, B32 - 7, B32, B32 + 3, B32 + (1 << 20) - 65495, (1 << 31) - 9, 5]
    lens = [65495, 1461, 14, 1460, 100, 65495, 18, 33]
    for at, n in zip(spots, lens):  # only the touched ranges are written (some sources overlap: that is allowed)
        big[at:at + n] = _dev(rng.integers(0, 256, n, dtype=np.uint8))
    want_src = {at: big[at:at + n].cpu().numpy() for at, n in zip(spots, lens)}
    dres = [3, 0, 9, 15, 1, 8, 4, 6]
    _, dst, _, nd = _packed(lens, [0] * len(lens), dres)
    ring = torch.full((nd,), SENT, dtype=torch.uint8, device="cuda:0")
    reng.copy_pieces(big, ring, _dev(_pieces(spots, dst, lens).view(np.uint8)))
    got = ring.cpu().numpy()
    want = np.full(nd, SENT, np.uint8)
    for at, d, n in zip(spots, dst, lens):
        want[d:d + n] = want_src[at]
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    for at, n in zip(spots, lens):
        assert (big[at:at + n].cpu().numpy() == want_src[at]).all()
    del big
    torch.cuda.empty_cache()


def test_grid_stride_second_trip(reng):
    """2^24 + 65 573 pieces of zero and one byte: the capped grid walks them in
    several trips with a 64-bit piece index"""
    torch = _torch()
    m = (1 << 24) + 65573
    i = torch.arange(m, dtype=torch.int64, device="cuda:0")
    pieces = torch.stack([i, i | ((i & 1) << 32)], dim=1).contiguous()  # src = dst = i, len = i & 1
    src = ((i * 37 + 11) & 0xFF).to(torch.uint8)
    dst = torch.full((m,), SENT, dtype=torch.uint8, device="cuda:0")
    reng.copy_pieces(src, dst, pieces.view(torch.uint8), m=m)
    odd = (i & 1).bool()
    assert bool((dst[odd] == src[odd]).all()) and bool((dst[~odd] == SENT).all())
    assert reng.dispatch_info()["kernel"] == "copy_pieces"
    del i, pieces, src, dst, odd
    torch.cuda.empty_cache()


def test_copy_call_level_errors(reng):
    from tcpip_network_protocol_stack_amd._lib import IcsumError

    torch = _torch()
    a = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    p = torch.zeros(32, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(IcsumError, match="null device buffer"):
        reng._check(reng.lib.ics_copy_pieces(reng.ctx, None, 0, a.data_ptr(), 64, p.data_ptr(), 1, None))
    with pytest.raises(IcsumError, match="not 8-byte aligned"):
        reng._check(reng.lib.ics_copy_pieces(reng.ctx, a.data_ptr(), 64, a.data_ptr(), 64, p.data_ptr() + 4, 1, None))
    with pytest.raises(IcsumError, match="above 2\\^31"):
        reng._check(reng.lib.ics_copy_pieces(reng.ctx, a.data_ptr(), 64, a.data_ptr(), (1 << 31) + 1, p.data_ptr(), 1,
                                             None))


# ---- end to end on the device -------------------------------------------------
MSG = {"src": 0x0A000001, "dst": 0x0A000002, "src_port": 4000, "dst_port": 80, "ackno": 0, "window": 1000,
       "ttl": 64, "id": 7}


def wire(op):
    """the datagram wrap_tcp_in_ip would put on the wire for a recv operation"""
    payload = payload_of(op)
    return wrap40(dict(MSG, seqno=op["seqno"], flags=flags_of(op)), payload) + payload


class DeviceDriver:
    """a batch of recv operations as wire datagrams in device memory:
    ics_tcp_unwrap_batch, the records to the host, receive_batch, read"""

    def __init__(self, eng, capacity, lead=0, stream=None):
        from tcpip_network_protocol_stack_amd.engine import TCP_RX_DTYPE

        self.eng, self.dtype, self.lead, self.stream = eng, TCP_RX_DTYPE, lead, stream
        self.rx = eng.rx_stream(capacity)

    def batch(self, ops, tag=""):
        torch = _torch()
        wires = [wire(o) for o in ops]
        off = np.zeros(len(wires) + 1, np.uint64)
        off[1:] = np.cumsum([len(w) for w in wires])
        with torch.cuda.stream(self.stream) if self.stream is not None else _null():
            buf = _dev(np.frombuffer(b"\x5b" * self.lead + b"".join(wires), np.uint8))[self.lead:]
            d_off = _dev(off.view(np.int64))
            recs = self.eng.tcp_unwrap_batch(buf, offsets=d_off, stream=self.stream)
            if self.stream is not None:
                self.stream.synchronize()
            recs = recs.cpu().numpy().view(self.dtype)
        assert (recs["status"] == 0x0F).all(), tag
        assert (recs["pay_len"] == [len(payload_of(o)) for o in ops]).all(), tag
        self.rx.receive(buf, recs, offsets=off, stream=self.stream)
        self.keep = buf  # alive until the next batch: the copy is only enqueued

    def pop(self, n):
        return self.rx.read(n, stream=self.stream)

    def set_error(self):
        self.rx.set_error()

    def answers(self):
        return lib_answers(self.rx)

    def close(self):
        _torch().cuda.synchronize()
        self.rx.close()


class _null:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize("how", ["each", "whole"])
def test_fixture_scenarios_on_the_device(reng, how):
    for i, sc in enumerate(load_golden()):
        drv = DeviceDriver(reng, sc["capacity"], lead=i % 4)
        run_scenario(drv, sc, how)
        drv.close()


def _burst(eng, cap, lead, stream=None, seed=1, nseg=3000):
    """a random stream of nseg datagrams against the restatement: every pop's
    bytes and the answers at every cut.  lead None: the datagram buffer's base
    moves through +0 .. +3 from batch to batch."""
    rng = random.Random(seed * 7919 + cap)
    ops = random_stream(rng, cap, ISNS[(cap + (lead or 0)) % len(ISNS)], nseg, pops=0.02)
    ref, drv = RefStream(cap), DeviceDriver(eng, cap, lead=lead or 0, stream=stream)
    popped = 0
    for k, item in enumerate(batches(ops, "whole")):
        if isinstance(item, list):
            for o in item:
                ref_apply(ref, o)
            if lead is None:
                drv.lead = k % 4
            drv.batch(item, (cap, k))
        else:
            want = ref_apply(ref, item)
            assert drv.pop(item["n"]) == want, (cap, lead, k)
            popped += len(want)
        assert drv.answers() == ref.answers(), (cap, lead, k)
    drv.close()
    return popped


@pytest.mark.parametrize("cap", [1000, 65535])
def test_random_burst(reng, cap):
    # 3000 datagrams, the buffer based at +0 .. +3 in turn; the ring wrapped
    # (what the restatement reads with this seed, computed on the CPU: 14 175 bytes at 1000, 219 582 at 65 535)
    assert _burst(reng, cap, None, nseg=3000) > cap


def test_non_default_stream(reng):
    torch = _torch()
    assert _burst(reng, 4096, 1, stream=torch.cuda.Stream(), nseg=300) > 4096


def test_two_streams_from_two_threads(reng):
    torch = _torch()
    errors = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            _burst(reng, (1000, 4096)[k], k, stream=torch.cuda.Stream(), seed=10 + k, nseg=400)
        except BaseException as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_receive_call_level_cases(reng):
    from tcpip_network_protocol_stack_amd._lib import IcsumError
    from tcpip_network_protocol_stack_amd.engine import TCP_RX_DTYPE, RxStream
    from rx_driver import recv

    drv = DeviceDriver(reng, 64)
    before = reng.dispatch_info()
    drv.rx.receive(None, np.zeros(0, TCP_RX_DTYPE))  # n = 0: nothing looked at, nothing launched
    assert reng.dispatch_info() == before
    ops = [recv(100, b"", syn=True), recv(101, b"abcdef")]
    drv.batch(ops[:1])  # a SYN alone: planned, no piece, k_copy_pieces not launched
    assert reng.dispatch_info()["kernel"] == "unwrap" and lib_answers(drv.rx)["ackno"] == 101
    drv.batch(ops[1:])
    assert reng.dispatch_info()["kernel"] == "copy_pieces"
    state = lib_answers(drv.rx)
    recs = np.zeros(1, TCP_RX_DTYPE)
    recs["status"], recs["pay_off"], recs["pay_len"] = 0x0F, 40, 7
    recs["msg"]["seqno"] = 107
    off = np.array([0, 46], np.uint64)
    with pytest.raises(IcsumError, match="outside its datagram of 46"):
        drv.rx.receive(drv.keep, recs, offsets=off)
    with pytest.raises(IcsumError, match="offsets decrease at datagram 0"):
        drv.rx.receive(drv.keep, recs, offsets=off[::-1].copy())
    with pytest.raises(IcsumError, match="null datagram buffer"):
        drv.rx.receive(None, recs, offsets=off)
    with pytest.raises(IcsumError, match="null records"):
        reng._check(reng.lib.ics_rx_stream_receive_batch(reng.ctx, drv.rx.handle, drv.keep.data_ptr(), None, 64, 46, 1,
                                                         None, None, None))
    with pytest.raises(IcsumError, match="null stream"):
        reng._check(reng.lib.ics_rx_stream_receive_batch(reng.ctx, None, drv.keep.data_ptr(), None, 64, 46, 1,
                                                         recs.ctypes.data, None, None))
    host_only = RxStream(64, debug="debug" in reng.lib.ics_version().decode())  # no ring: the device calls refuse it
    host_only.engine = reng
    with pytest.raises(IcsumError, match="without a ring"):
        host_only.receive(drv.keep, recs, offsets=off)
    with pytest.raises(IcsumError, match="without a ring"):
        host_only.read(4)
    host_only.close()
    assert lib_answers(drv.rx) == state  # refused calls change nothing
    assert drv.pop(64) == b"abcdef"
    assert drv.rx.ring() != 0
    drv.close()


def test_verify_and_unwrap_are_unchanged_around_a_receive_call(reng):
    torch = _torch()
    rng = random.Random(3)
    ops = random_stream(rng, 4096, 5, 300, pops=0.0)
    recvs = [o for o in ops if o["op"] == "recv"]
    wires = [wire(o) for o in recvs]
    off = np.zeros(len(wires) + 1, np.uint64)
    off[1:] = np.cumsum([len(w) for w in wires])
    buf, d_off = _dev(np.frombuffer(b"".join(wires), np.uint8)), _dev(off.view(np.int64))

    def both():
        ip, tcp, st = reng.ipv4_tcp_batch(buf, 1, offsets=d_off)
        k1 = reng.dispatch_info()
        recs = reng.tcp_unwrap_batch(buf, offsets=d_off)
        k2 = reng.dispatch_info()
        return [t.cpu().numpy().copy() for t in (ip, tcp, st, recs)], [(k[x]) for k in (k1, k2) for x in
                                                                      ("kernel", "lps", "unroll", "plan")]

    out_a, launch_a = both()
    rx = reng.rx_stream(4096)
    rx.receive(buf, out_a[3].view(rx_dtype()), offsets=off)
    assert reng.dispatch_info()["kernel"] == "copy_pieces"
    out_b, launch_b = both()
    assert launch_a == launch_b
    for a, b in zip(out_a, out_b):
        assert (a == b).all()
    torch.cuda.synchronize()
    rx.close()


def rx_dtype():
    from tcpip_network_protocol_stack_amd.engine import TCP_RX_DTYPE

    return TCP_RX_DTYPE


def test_batch_engine_receive_records():
    """csrc/host/tests/rx_stream_gpu_test.cpp: BatchEngine::receive_records
    (records, gates from record fields, the copy on the device) against the
    per-object unwrap_tcp_in_ip gates and a host-only RxStream's plan applied on
    the host, batch for batch"""
    import os
    import subprocess

    from conftest import ROOT

    exe = os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc", "host", "build", "rx_stream_gpu_test")
    assert os.path.exists(exe), "build() did not produce rx_stream_gpu_test"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.startswith("OK:")
