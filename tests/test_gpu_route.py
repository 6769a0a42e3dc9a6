"""GPU: Router::match on the device — the lookup-only batch
(ics_route_lookup_batch, k_route_lookup) and the lookup fused into both router
kernels (ics_router_route_batch / ics_router_route_headers), i.e.
Router::route whole (the reference's src/router/router.cpp:27-70).

References: for the route answers, RouteTable.match and the Python restatement
of Router::match (route_ref.py), both pinned to the real reference's answers in
test_route_table.py; for the forward decision and every byte written, the
existing router calls (router_ttl_headers / router_ttl_batch, themselves pinned
to the reference) on the same input — the fused calls must leave exactly their
bytes whether or not a route exists.  Every test runs in the release build and
in libicsum_debug.so, whose kernels check every trie and record index against
the image (a violation fails the call).  Bar: exact."""
import ctypes

import numpy as np
import pytest

from conftest import engine_with
from helpers import pack_contiguous
from route_ref import NO_ROUTE, RefRouter, boundary_addrs, fill, random_routes
from test_gpu_parity import _random_datagrams, _t, _u32

pytestmark = pytest.mark.gpu

# every trie level, a dead route, an overwritten one, a next hop of 0.0.0.0; no default route
ROUTES = [
    (0x0A000000, 8, 1, False, 0),            # level 1 leaves
    (0x0A010000, 16, 2, True, 0x01010101),
    (0x0A010200, 24, 3, False, 0),           # level 2
    (0x0A010240, 26, 4, True, 0),            # level 3; next hop 0.0.0.0 is a next hop
    (0x0A010242, 31, 5, False, 0),
    (0xC0A80000, 17, 6, False, 0),
    (0xC0A88001, 17, 7, False, 0),           # host bit set: dead
    (0xAC100000, 12, 8, True, 0x02020202),
    (0x0A010200, 24, 9, True, 0x03030303),   # replaces interface 3
    (0x0A020000, 15, 10, False, 0),
]
REF = RefRouter(ROUTES)
POOL = np.array(boundary_addrs(ROUTES) + [0, 1, 0xFFFFFFFF, 0x0B000000, 0x7F000001, 0xE0000001], dtype=np.uint32)


@pytest.fixture(scope="module", params=[False, True], ids=["release", "debug"])
def rt(request):
    """(engine, RouteTable of ROUTES) of one library build"""
    from tcpip_network_protocol_stack_amd.engine import RouteTable

    gen = engine_with(None, debug=request.param)
    eng = next(gen)
    table = fill(RouteTable(debug=request.param), ROUTES)
    yield eng, table
    next(gen, None)
    table.close()


def _sentinel(n, dtype, value):
    import torch

    return torch.full((n,), value, dtype=dtype, device="cuda:0")


def _want(ref, fwd, dsts):
    """(status, iface, next_hop) for forward flags and each datagram's dst"""
    m, f, h = ref.answers(dsts)
    routed = fwd & m
    return (fwd.astype(np.uint8) | (routed.astype(np.uint8) << 1), np.where(routed, f, NO_ROUTE).astype(np.uint32),
            np.where(routed, h, 0).astype(np.uint32))


def _dsts(buf, off):
    """host-order dst of every datagram (0 where it is shorter than a header)"""
    out = np.zeros(off.size - 1, dtype=np.uint32)
    for i in range(off.size - 1):
        a, b = int(off[i]), int(off[i + 1])
        if b - a >= 20:
            out[i] = int.from_bytes(buf[a + 16:a + 20].tobytes(), "big")
    return out


# ------------------------------------------------------------ lookup batch --
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2051])
def test_lookup_batch(rt, n):
    import torch

    eng, table = rt
    rng = np.random.default_rng(0x100 + n)
    addrs = np.concatenate([POOL, rng.integers(0, 2**32, 2051, dtype=np.uint64).astype(np.uint32)])
    addrs = addrs[rng.permutation(addrs.size)][:n] if n > 1 else np.array([0x0A010243], dtype=np.uint32)
    f, h = _sentinel(n, torch.int32, 0x25A5A5A5), _sentinel(n, torch.int32, 0x25A5A5A5)
    eng.route_lookup_batch(table, _t(addrs), iface=f, next_hop=h)
    assert eng.dispatch_info()["kernel"] == "route_lookup"
    m, wf, wh = REF.answers(addrs)
    assert (_u32(f) == wf).all() and (_u32(h) == wh).all()
    for k in range(min(n, 200)):  # and RouteTable.match, the same image walked on the host
        got = table.match(int(addrs[k]))
        assert (got is not None) == bool(m[k]) and (got is None or got == (wf[k], wh[k]))
    if n > 60:
        assert 0 < m.sum() < n
    # either output absent
    f2 = _sentinel(n, torch.int32, 0x25A5A5A5)
    lib, st = eng.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    eng._check(lib.ics_route_lookup_batch(eng.ctx, table.handle, _t(addrs).data_ptr(), n, f2.data_ptr(), None, st))
    assert (_u32(f2) == wf).all()


def test_lookup_batch_tables(rt):
    """an empty table (all unmatched), then a 300-route random table with
    every level populated, through the same context"""
    import torch

    from tcpip_network_protocol_stack_amd.engine import RouteTable

    eng, table = rt
    debug = table.debug
    rng = np.random.default_rng(0x7AB)
    addrs = np.concatenate([POOL, rng.integers(0, 2**32, 500, dtype=np.uint64).astype(np.uint32)])
    empty = RouteTable(debug=debug)
    f, h = eng.route_lookup_batch(empty, _t(addrs))
    assert (_u32(f) == NO_ROUTE).all() and (_u32(h) == 0).all()
    routes = random_routes(rng, 300)
    big = fill(RouteTable(debug=debug), routes)
    assert big.stats()["l3_chunks"] > 0
    addrs = np.array(boundary_addrs(routes)[:2500] + [int(a) for a in rng.integers(0, 2**32, 500)], dtype=np.uint32)
    f, h = eng.route_lookup_batch(big, _t(addrs))
    m, wf, wh = RefRouter(routes).answers(addrs)
    assert (_u32(f) == wf).all() and (_u32(h) == wh).all()
    f, h = eng.route_lookup_batch(table, _t(POOL))  # the first table again: its image is still the context's
    _, wf, wh = REF.answers(POOL)
    assert (_u32(f) == wf).all() and (_u32(h) == wh).all()
    torch.cuda.synchronize()
    empty.close()
    big.close()


# ------------------------------------------------------------ fused router --
@pytest.fixture(scope="module")
def arena(orc):
    """The input of test_router_headers_random (3000 datagrams: every ttl,
    hlen 6, the reserved flag bit, bad checksums, shorter than 20 bytes) with
    the valid headers' dst drawn from a pool that hits every trie level and
    misses.  Shared, never written."""
    rng = np.random.default_rng(15)
    segs = _random_datagrams(rng, 3000)
    pick = np.random.default_rng(16).integers(0, POOL.size, len(segs))
    for i in range(0, len(segs), 2):
        if len(segs[i]) >= 20:
            b = bytearray(segs[i])
            b[0] = 0x45 if i % 10 else 0x46
            b[6] |= 0x80 if i % 6 == 0 else 0
            b[8] = i % 256
            b[16:20] = int(POOL[pick[i]]).to_bytes(4, "big")
            _, _, _, b = orc.ipv4_tcp(bytes(b), 2)
            segs[i] = b
    buf, off = pack_contiguous(segs, 1)
    return buf, off, _dsts(buf, off)


def _fused_headers(eng, table, d, n, **kw):
    import torch

    hd, st = _sentinel(n * 20, torch.uint8, 0xA5), _sentinel(n, torch.uint8, 0x5A)
    f, h = _sentinel(n, torch.int32, 0x25A5A5A5), _sentinel(n, torch.int32, 0x25A5A5A5)
    eng.router_route_headers(table, d, n=n, hdrs=hd, status=st, iface=f, next_hop=h, **kw)
    assert eng.dispatch_info()["kernel"] == "router_route_hdrs"
    return hd.cpu().numpy(), st.cpu().numpy(), _u32(f), _u32(h)


def _fused_in_place(eng, table, d, n, **kw):
    import torch

    st = _sentinel(n, torch.uint8, 0x5A)
    f, h = _sentinel(n, torch.int32, 0x25A5A5A5), _sentinel(n, torch.int32, 0x25A5A5A5)
    eng.router_route_batch(table, d, n=n, status=st, iface=f, next_hop=h, **kw)
    assert eng.dispatch_info()["kernel"] == "router_route"
    return st.cpu().numpy(), _u32(f), _u32(h)


def _check_both_forms(eng, table, ref, buf, dsts, n, tag, place=_t, **kw):
    """headers apart, then in place, on fresh copies of `buf`, against the
    existing router calls on the same bytes and the restatement on each dst;
    returns the wanted status"""
    d = place(buf)
    hd0, st0 = eng.router_ttl_headers(d, n=n, **kw)
    hd0, fwd = hd0.cpu().numpy(), st0.cpu().numpy().astype(bool)
    want_st, want_f, want_h = _want(ref, fwd, dsts)
    hd, st, f, h = _fused_headers(eng, table, d, n, **kw)
    assert (st == want_st).all() and (hd == hd0).all(), tag
    assert (f == want_f).all() and (h == want_h).all(), tag
    assert (d.cpu().numpy() == buf).all(), tag  # the input stays unwritten
    d1, d2 = place(buf), place(buf)
    st1 = eng.router_ttl_batch(d1, n=n, **kw).cpu().numpy()
    assert (st1.astype(bool) == fwd).all(), tag
    st, f, h = _fused_in_place(eng, table, d2, n, **kw)
    assert (st == want_st).all() and (d2.cpu().numpy() == d1.cpu().numpy()).all(), tag
    assert (f == want_f).all() and (h == want_h).all(), tag
    return want_st


def test_fused_random_batch(rt, arena):
    eng, table = rt
    buf, off, dsts = arena
    n = off.size - 1
    want_st = _check_both_forms(eng, table, REF, buf, dsts, n, "random", offsets=_t(off))
    # forwarded and routed, forwarded with no route, dropped: all present
    assert (want_st == 3).sum() > 0 and (want_st == 1).sum() > 0 and (want_st == 0).sum() > 0
    assert set(np.unique(want_st)) == {0, 1, 3}
    m, f, _ = REF.answers(dsts[want_st == 3])
    assert {1, 2, 4, 5, 6, 8, 9, 10} <= set(f.tolist())  # every live route of every trie level was an answer


def _fixed_batch(orc, stride, n):
    rng = np.random.default_rng(0x5D + stride)
    buf = rng.integers(0, 256, n * stride, dtype=np.uint8)
    pick = rng.integers(0, POOL.size, n)
    for i in range(n):
        b = bytearray(buf[i * stride:(i + 1) * stride].tobytes())
        b[0] = 0x45
        b[2], b[3] = stride >> 8, stride & 0xFF
        b[6] = (b[6] | 0x80) if i % 3 == 0 else (b[6] & 0x7F)
        b[8] = i % 256
        b[16:20] = int(POOL[pick[i]]).to_bytes(4, "big")
        if i % 5 != 4:  # every fifth header keeps a wrong checksum (dropped)
            _, _, _, b = orc.ipv4_tcp(bytes(b), 2)
        buf[i * stride:(i + 1) * stride] = np.frombuffer(bytes(b), dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * stride
    return buf, _dsts(buf, off)


@pytest.mark.parametrize("stride", [20, 64, 1500, 1502])
def test_fused_fixed_stride(rt, orc, stride):
    eng, table = rt
    n = 2051  # not a multiple of a wave's 32 datagrams
    buf, dsts = _fixed_batch(orc, stride, n)
    want_st = _check_both_forms(eng, table, REF, buf, dsts, n, stride, stride=stride, dgram_len=stride)
    assert (want_st == 3).sum() > 0 and (want_st == 1).sum() > 0 and (want_st == 0).sum() > 0


@pytest.mark.parametrize("base", [1, 2, 3, 14])
def test_fused_any_base(rt, arena, base):
    """packed offsets with odd starts, the batch 1, 2, 3 and 14 bytes into its allocation"""
    from test_gpu_base_align import _place, _untouched

    eng, table = rt
    buf, off, dsts = arena
    n = 700
    end = int(off[n])
    wholes = []

    def place(b):
        view, whole = _place(b, base)
        wholes.append(whole)
        return view

    _check_both_forms(eng, table, REF, buf[:end], dsts[:n], n, base, place=place, offsets=_t(off[:n + 1]))
    for w in wholes:
        _untouched(w, base, end)


def test_fused_single_datagram_and_absent_outputs(rt, orc, arena):
    import torch

    eng, table = rt
    buf, dsts = _fixed_batch(orc, 64, 40)
    one = buf[128:192].copy()  # datagram 2: ttl 2, a valid checksum
    want_st = _check_both_forms(eng, table, REF, one, dsts[2:3], 1, "n=1", stride=64, dgram_len=64)
    assert want_st[0] in (1, 3)
    # d_iface / d_next_hop absent, independently; n == 0 launches nothing
    n = 40
    fwd = eng.router_ttl_headers(_t(buf), n=n, stride=64, dgram_len=64)[1].cpu().numpy().astype(bool)
    want_st, want_f, want_h = _want(REF, fwd, dsts)
    lib, stream = eng.lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_f, with_h in ((True, False), (False, True), (False, False)):
        d = _t(buf)
        hd, st = _sentinel(n * 20, torch.uint8, 0xA5), _sentinel(n, torch.uint8, 0x5A)
        f, h = _sentinel(n, torch.int32, 0x25A5A5A5), _sentinel(n, torch.int32, 0x25A5A5A5)
        eng._check(lib.ics_router_route_headers(eng.ctx, table.handle, d.data_ptr(), None, 64, 64, n, hd.data_ptr(),
                                                st.data_ptr(), f.data_ptr() if with_f else None,
                                                h.data_ptr() if with_h else None, stream))
        assert (st.cpu().numpy() == want_st).all()
        assert (_u32(f) == (want_f if with_f else 0x25A5A5A5)).all()
        assert (_u32(h) == (want_h if with_h else 0x25A5A5A5)).all()
        st2 = _sentinel(n, torch.uint8, 0x5A)
        eng._check(lib.ics_router_route_batch(eng.ctx, table.handle, d.data_ptr(), None, 64, 64, n, st2.data_ptr(),
                                              f.data_ptr() if with_f else None, h.data_ptr() if with_h else None,
                                              stream))
        assert (st2.cpu().numpy() == want_st).all()
    before = eng.dispatch_info()["kernel"]
    assert lib.ics_router_route_batch(eng.ctx, table.handle, None, None, 64, 64, 0, None, None, None, stream) == 0
    assert lib.ics_route_lookup_batch(eng.ctx, table.handle, None, 0, None, None, stream) == 0
    assert eng.dispatch_info()["kernel"] == before
    assert lib.ics_router_route_batch(eng.ctx, None, d.data_ptr(), None, 64, 64, n, st2.data_ptr(), None, None,
                                      stream) == -1
    assert b"null route table" in lib.ics_last_error()
    assert lib.ics_router_route_headers(eng.ctx, table.handle, d.data_ptr(), None, 64, 64, n, None, st2.data_ptr(),
                                        None, None, stream) == -1


def test_table_change_is_seen_by_the_next_call(rt):
    """two calls on one stream around a table change: a more specific route
    added, then clear"""
    from tcpip_network_protocol_stack_amd.engine import RouteTable

    eng, table = rt
    t = RouteTable(debug=table.debug)
    t.add(0x0A000000, 8, 1)
    addrs = np.array([0x0A010203, 0x0A010303, 0x0B000000], dtype=np.uint32)
    d = _t(addrs)
    f, h = eng.route_lookup_batch(t, d)
    assert _u32(f).tolist() == [1, 1, NO_ROUTE] and _u32(h).tolist() == [0x0A010203, 0x0A010303, 0]
    t.add(0x0A010200, 25, 2, next_hop=7)
    f, h = eng.route_lookup_batch(t, d)
    assert _u32(f).tolist() == [2, 1, NO_ROUTE] and _u32(h).tolist() == [7, 0x0A010303, 0]
    t.clear()
    f, h = eng.route_lookup_batch(t, d)
    assert _u32(f).tolist() == [NO_ROUTE] * 3 and _u32(h).tolist() == [0] * 3
    t.close()


def test_more_tables_than_image_slots(rt):
    """six tables through a context that keeps four images: the least recently
    used image is replaced and uploaded again when its table comes back"""
    from tcpip_network_protocol_stack_amd.engine import RouteTable

    eng, table = rt
    rng = np.random.default_rng(0x51075)
    sets = [random_routes(rng, 40 + 30 * k) for k in range(6)]
    tables = [fill(RouteTable(debug=table.debug), r) for r in sets]
    refs = [RefRouter(r) for r in sets]
    probes = [np.array(boundary_addrs(r)[:600] + [int(a) for a in rng.integers(0, 2**32, 100)], dtype=np.uint32)
              for r in sets]
    for k in [0, 1, 2, 3, 4, 5, 0, 2, 5, 1, 3, 3, 4]:
        f, h = eng.route_lookup_batch(tables[k], _t(probes[k]))
        _, wf, wh = refs[k].answers(probes[k])
        assert (_u32(f) == wf).all() and (_u32(h) == wh).all(), k
    f, h = eng.route_lookup_batch(table, _t(POOL))  # the module's table, evicted meanwhile
    _, wf, wh = REF.answers(POOL)
    assert (_u32(f) == wf).all() and (_u32(h) == wh).all()
    for t in tables:
        t.close()


# --------------------------------------------------------- batch-size sweep --
def test_lookup_every_batch_size(rt):
    """n = 0..130, 255..257, 511..513 on one uploaded batch: a partial last wave of every size, the block edge"""
    import torch
    import periodic as P

    eng, table = rt
    rng = np.random.default_rng(0x5EE9)
    addrs = np.concatenate([POOL, rng.integers(0, 2**32, P.SWEEP_MAX, dtype=np.uint64).astype(np.uint32)])
    addrs = addrs[rng.permutation(addrs.size)][:P.SWEEP_MAX]
    m, wf, wh = REF.answers(addrs)
    assert 0 < m[:64].sum() < 64
    d = _t(addrs)
    P.sweep_sizes(lambda n, o: eng.route_lookup_batch(table, d, n=n, iface=o[0], next_hop=o[1]),
                  [(torch.int32, 1, 0x25A5A5A5)] * 2, [wf, wh])


def test_fused_headers_every_batch_size(rt, arena):
    """router_route_headers (two lanes per datagram: 32 datagrams a wave, 128 a block) at the same sizes, on the
    first n datagrams of the shared arena, against the restatement"""
    import torch
    import periodic as P

    eng, table = rt
    buf, off, _ = arena
    n = P.SWEEP_MAX
    dgrams = [buf[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    st, fi, fh, hd, _ = P.route_expect(dgrams, REF)
    assert set(np.unique(st[:32])) == {0, 1, 3}
    d, doff = _t(buf), _t(off[:n + 1])
    P.sweep_sizes(lambda k, o: eng.router_route_headers(table, d, n=k, offsets=doff, hdrs=o[0], status=o[1], iface=o[2],
                                                        next_hop=o[3]),
                  [(torch.uint8, 20, 0xA5), (torch.uint8, 1, 0x5A), (torch.int32, 1, 0x25A5A5A5),
                   (torch.int32, 1, 0x25A5A5A5)], [hd, st, fi, fh])
    assert (d.cpu().numpy() == buf).all()
