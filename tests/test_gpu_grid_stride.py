"""GPU: the second grid-stride trip of the route, frame and unwrap kernels.

`ew_blocks` caps every element-wise grid at 65 536 blocks of 256 threads, so
k_frame, k_tcp_unwrap and k_route_lookup take a second trip of their
`for (g0 ...; g0 += step)` loop only above 2^24 items, and the fused router
kernels (two lanes per datagram) above 2^23 datagrams.  What runs only there:
the wave's LDS rows rewritten behind the trailing wave_barrier, k_tcp_unwrap's
rows reused as the record staging area, and the 64-bit `wbase * kRec + t` store
index.  The family suites stop at 2^18 + 3.

Batches: periodic.py's K = 4099 items, uploaded once and repeated on the device
(`Tensor.repeat`; K is prime, so the period never lines up with a wave, a block
or the grid) to n = 2^24 + 65 573 items — a second trip of 256 full blocks and
one partial wave of 37 — and n = 2^23 + 32 805 datagrams for the two-lane router
kernels (256 blocks of 128 datagrams and 37).  The expectation is the K-item
restatement (frame_ref / route_ref / unwrap_ref) repeated the same way and
compared with torch.equal over the whole output, 64 sentinel elements behind
every output.  Every status class is asserted present in the K items.  Bar:
exact.

Power check (once, scratch builds, not kept): with each loop ended after its
first trip (`break` before the closing brace in k_frame, k_tcp_unwrap,
k_route_lookup, k_router_hdrs and k_router_ttl) every test of this module fails
at its first comparison with the outputs' 0x5A / 0x25A5A5A5 / 0xA5 sentinel in
the first differing element, and the earlier suites (test_gpu_route,
test_gpu_frames, test_gpu_unwrap) pass unchanged."""
import numpy as np
import pytest

import periodic as P
from conftest import engine_with
from frame_ref import RefNeigh
from route_ref import RefRouter, fill
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

N1 = (1 << 24) + 65573  # one lane per item
N2 = (1 << 23) + 32805  # two lanes per datagram
S8, S32, SREC = 0x5A, 0x25A5A5A5, 0xA5


@pytest.fixture(scope="module")
def gs():
    """(engine, RouteTable, NeighTable, RefRouter, RefNeigh): test_gpu_frames' tables"""
    import test_gpu_frames as F
    from tcpip_network_protocol_stack_amd.engine import NeighTable, RouteTable

    gen = engine_with(None)
    eng = next(gen)
    routes, neigh = fill(RouteTable(), F.ROUTES), F._fill_neigh(NeighTable())
    yield eng, routes, neigh, RefRouter(F.ROUTES), F._fill_neigh(RefNeigh())
    next(gen, None)
    routes.close()
    neigh.close()


def _same(got_whole, n, want, sent, tag):
    """the first n elements equal `want`, the tail is untouched; on a mismatch name the first element"""
    import torch

    got = got_whole[:n]
    if not torch.equal(got, want):
        i = int((got != want).nonzero()[0])
        raise AssertionError(f"{tag}: element {i} (of {n}) is {int(got[i]):#x}, want {int(want[i]):#x}")
    assert P.tail_untouched(got_whole, n, sent), f"{tag}: written behind the output"


def test_frames_past_the_grid_cap(gs):
    import torch
    import test_gpu_frames as F

    eng, routes, neigh, router, rneigh = gs
    n = N1
    frames, ins = P.frame_items()
    st, fi, fh, rec = F.expect(frames, ins, router, rneigh)
    P.assert_frame_classes(st)
    d = P.tile(_t(P.frames_fixed(frames)), n, P.FRAME_STRIDE)
    dins = P.tile(_t(ins), n)
    kw = dict(n=n, stride=P.FRAME_STRIDE, frame_len=P.FRAME_LEN, in_ifaces=dins)
    w_st0, st0 = P.sentinel(n, torch.uint8, S8)
    eng.frame_recv(neigh, d, status=st0, **kw)
    assert eng.dispatch_info()["kernel"] == "frame_recv"
    _same(w_st0, n, P.tile(_t(st & 0xF8), n), S8, "frame_recv status")
    del w_st0, st0
    (w_hd, hd), (w_st, s) = P.sentinel(n * 36, torch.uint8, SREC), P.sentinel(n, torch.uint8, S8)
    (w_f, f), (w_h, h) = P.sentinel(n, torch.int32, S32), P.sentinel(n, torch.int32, S32)
    eng.router_frames(routes, neigh, d, hdrs=hd, status=s, iface=f, next_hop=h, **kw)
    assert eng.dispatch_info()["kernel"] == "router_frames"
    _same(w_st, n, P.tile(_t(st), n), S8, "router_frames status")
    _same(w_f, n, P.tile(_t(fi), n), S32, "router_frames iface")
    _same(w_h, n, P.tile(_t(fh), n), S32, "router_frames next_hop")
    _same(w_hd, n * 36, P.tile(_t(rec.reshape(-1)), n, 36), SREC, "router_frames records")


@pytest.mark.parametrize("with_status", [True, False], ids=["status", "scratch"])
def test_unwrap_past_the_grid_cap(gs, with_status):
    import torch

    eng = gs[0]
    n = N1
    dgrams = P.unwrap_items()
    want = P.unwrap_expect(dgrams)
    P.assert_unwrap_classes(want, dgrams)
    buf, off = P.pack(dgrams)
    doff = P.tile_offsets(off, n)
    d = _t(buf).repeat(-(-n // P.K))[:int(doff[n])]
    w_rec, rec = P.sentinel(n * 40, torch.uint8, SREC)
    w_st, st = P.sentinel(n, torch.uint8, S8) if with_status else (None, None)
    eng.tcp_unwrap_batch(d, n=n, offsets=doff, recs=rec, status=st)
    assert eng.dispatch_info()["kernel"] == "unwrap"
    _same(w_rec, n * 40, P.tile(_t(want.reshape(-1)), n, 40), SREC, "unwrap records")
    if with_status:
        _same(w_st, n, P.tile(_t(want[:, 36].copy()), n), S8, "unwrap status")


def test_lookup_past_the_grid_cap(gs):
    import torch
    import test_gpu_frames as F

    eng, routes, _, router, _ = gs
    n = N1
    addrs = P.addr_items(F.ROUTES)
    m, wf, wh = router.answers(addrs)
    assert 0 < m.sum() < P.K and {0, 1, 2, 3, 9} <= set(wf.tolist())
    (w_f, f), (w_h, h) = P.sentinel(n, torch.int32, S32), P.sentinel(n, torch.int32, S32)
    eng.route_lookup_batch(routes, P.tile(_t(addrs), n), n=n, iface=f, next_hop=h)
    assert eng.dispatch_info()["kernel"] == "route_lookup"
    _same(w_f, n, P.tile(_t(wf), n), S32, "lookup iface")
    _same(w_h, n, P.tile(_t(wh), n), S32, "lookup next_hop")


@pytest.mark.parametrize("in_place", [False, True], ids=["headers", "in_place"])
def test_fused_router_past_the_grid_cap(gs, in_place):
    import torch

    eng, routes, _, router, _ = gs
    n = N2
    dgrams = P.dgram_items()
    st, fi, fh, hd, after = P.route_expect(dgrams, router)
    P.assert_route_classes(st)
    buf, off = P.pack(dgrams)
    doff = P.tile_offsets(off, n)
    reps, end = -(-n // P.K), int(doff[n])
    w_d = torch.full((end + 64,), SREC, dtype=torch.uint8, device="cuda:0")
    w_d[:end] = _t(buf).repeat(reps)[:end]
    (w_st, s) = P.sentinel(n, torch.uint8, S8)
    (w_f, f), (w_h, h) = P.sentinel(n, torch.int32, S32), P.sentinel(n, torch.int32, S32)
    if in_place:
        eng.router_route_batch(routes, w_d[:end], n=n, offsets=doff, status=s, iface=f, next_hop=h)
        assert eng.dispatch_info()["kernel"] == "router_route"
        _same(w_d, end, _t(P.pack(after)[0]).repeat(reps)[:end], SREC, "datagram bytes after the in-place call")
    else:
        w_hd, hdrs = P.sentinel(n * 20, torch.uint8, SREC)
        eng.router_route_headers(routes, w_d[:end], n=n, offsets=doff, hdrs=hdrs, status=s, iface=f, next_hop=h)
        assert eng.dispatch_info()["kernel"] == "router_route_hdrs"
        _same(w_hd, n * 20, P.tile(_t(hd.reshape(-1)), n, 20), SREC, "forwarded headers")
        _same(w_d, end, _t(buf).repeat(reps)[:end], SREC, "datagram bytes (only read)")
    _same(w_st, n, P.tile(_t(st), n), S8, "status")
    _same(w_f, n, P.tile(_t(fi), n), S32, "iface")
    _same(w_h, n, P.tile(_t(fh), n), S32, "next_hop")
