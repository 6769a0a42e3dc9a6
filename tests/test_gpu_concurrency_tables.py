"""GPU: one engine context, several streams, the route and neighbour images.

INTEGRATION.md §5: "one context may serve several streams at once".  The
context keeps the compiled images of up to kRouteSlots = 4 route tables and 4
neighbour tables on the device and overwrites a slot's buffer in place when its
table's generation moved, when the LRU re-keys it for another table, and when
it grows.  Such an overwrite must wait for every launch that may still read
the slot, on any stream; readers of an unchanged image never wait for each
other.

test_threads_streams_and_tables (the shape of test_gpu_concurrency.py's test):
4 host threads, each on its own stream, 12 rounds, outputs reset to 0x5A each
round; per round route_lookup_batch, router_route_headers and the in-place
router_route_batch (each on its own copy of the datagrams), frame_recv,
router_frames, and tcp_unwrap_batch without a status array (the unwrap_status
lease nested over the scratch lease of its VERIFY launch) and with one — 5 x
4099 = 20 495 items each (periodic.py).  Six route tables and six neighbour
tables over the four threads, two per thread in turn, threads 0 and 1 sharing
pair 0: more tables than slots, so slots are re-keyed while other threads'
launches are in flight; no table changes during the rounds.  Every output of
every round must equal the same calls made one at a time on one stream, and
those serial results are compared in full with route_ref / frame_ref /
unwrap_ref.  Bar: bit-exact.

test_image_is_not_replaced_under_another_streams_launch (deterministic, two
streams, no threads; once for the route image through route_lookup_batch, once
for the neighbour image through router_frames):
  1. stream A: CALLS calls of ITEMS items reading table T, each into its own outputs;
  2. stream B: one call of 64 items on T;
  3. T changes so that every answer changes and the image's structure does
     not (every prefix re-added with another interface and next hop, every
     neighbour re-learnt with another address; stats() asserted unmoved: a
     launch that saw a mix of both images would still read valid indices only);
  4. stream B: the same 64-item call, which uploads the new image;
  5. synchronise: every output of A equals the old table's restatement in
     full, B's first call the old one, B's second the new one.
`evicted`: instead of 3-4, four other tables of the same structure take stream
B through the slots, so T's slot is re-keyed while A still reads it (all five
went through the slots before A started, so that no slot allocates its buffer
on the way and the fourth call is the one that takes T's slot).
A's queue is sized from a measurement on the parent commit (device events
around one of A's launches, seven repeats; time.perf_counter around steps 2-4):
  route:  one 2^24-address launch 64-70 us (median 65), steps 2-4 137 us on an
          idle device and 81 us with A's queue in flight; CALLS = 48 is a queue
          of 2983 us, 22 x the host path
  neigh:  one 2^22-frame launch 122-134 us (median 122), steps 2-4 68 us idle
          and 34 us with A in flight; CALLS = 24 is a queue of 2849 us, 42 x
The test asserts that A was still busy when step 3 had finished, and picks for
B a stream that is seen to run beside A (_stream_beside: the runtime places its
streams on a few hardware queues, and two streams on one queue run one behind
the other, which hides the hazard).

Power check (once, not kept): against the parent commit's libicsum.so - one
event per slot, re-recorded by whichever stream launched last - all four cases
fail, in both orders of running them: [route-changed] from A's call 6 on
(3 969 339 of 2^24 interfaces are the new table's), [route-evicted] from call
4 or 5 (the other table's answers), [neigh-changed] and [neigh-evicted] from
call 2 (records carrying the other addresses); B's calls are right.  With the
per-stream reader set of this change all pass, and step 4 takes as long as A's
queue (2652 us measured) instead of 81 us: it waits."""
import threading

import numpy as np
import pytest

import periodic as P
from conftest import engine_with
from frame_ref import RefNeigh
from route_ref import RefRouter, fill, random_routes
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

THREADS, ROUNDS, TABLES = 4, 12, 6
PAIRS = [(0, 1), (0, 2), (3, 4), (5, 3)]  # thread t uses table pair PAIRS[t][round % 2]
N = 5 * P.K


@pytest.fixture(scope="module")
def ceng():
    gen = engine_with(None)
    yield next(gen)
    next(gen, None)


# ------------------------------------------------------------------ tables --
def _routes_k(k):
    """test_gpu_frames' routes with the egress interfaces rotated by k, and 20 k random routes behind them"""
    import test_gpu_frames as F

    rot = [(p, ln, (f + k) % 4 if f < 4 else f, has, hop) for p, ln, f, has, hop in F.ROUTES]
    return rot + random_routes(np.random.default_rng(0x70 + k), 20 * k, lengths=list(range(9, 32)))


def _fill_neigh_k(t, k):
    """test_gpu_frames' interfaces and neighbours, every neighbour's address a function of k, 50 k more mappings"""
    import test_gpu_frames as F

    for i in F.MACS:
        t.set_iface(i, F.MACS[i], F.IPS[i])
    for f, ip in F.NEIGH:
        t.learn(f, ip, F._nmac(f, ip ^ k))
    for ip in np.random.default_rng(0x90 + k).integers(0, 2**32, 50 * k):
        t.learn(int(ip) % 4, int(ip), F._nmac(k, int(ip)))
    return t


# ----------------------------------------------------------------- A1 -----
class Job:
    """one thread's device inputs, outputs and calls"""

    def __init__(self, eng, tid):
        import torch

        self.eng = eng
        seed = 0xA100 + 16 * tid
        self.frames, self.ins = P.frame_items(seed)
        self.dgrams = P.dgram_items(seed + 1)
        self.unwraps = P.unwrap_items(seed + 2)
        self.addrs = P.addr_items(_routes_k(0), seed + 3)
        self.d_frames = P.tile(_t(P.frames_fixed(self.frames)), N, P.FRAME_STRIDE)
        self.d_ins = P.tile(_t(self.ins), N)
        buf, off = P.pack(self.dgrams)
        self.d_dgoff = P.tile_offsets(off, N)
        self.dg_end = int(self.d_dgoff[N])
        self.d_dg = _t(buf).repeat(5)
        self.d_dg_work = self.d_dg.clone()
        buf, off = P.pack(self.unwraps)
        self.d_uoff = P.tile_offsets(off, N)
        self.d_u = _t(buf).repeat(5)
        self.d_addrs = P.tile(_t(self.addrs), N)
        u8, i32 = torch.uint8, torch.int32
        shapes = [(N, i32), (N, i32),                              # 0-1  lookup
                  (N * 20, u8), (N, u8), (N, i32), (N, i32),       # 2-5  headers apart
                  (N, u8), (N, i32), (N, i32),                     # 6-8  in place
                  (N, u8),                                         # 9    frame_recv
                  (N * 36, u8), (N, u8), (N, i32), (N, i32),       # 10-13 router_frames
                  (N * 40, u8),                                    # 14   unwrap, status to the context's scratch
                  (N * 40, u8), (N, u8)]                           # 15-16 unwrap with a status array
        self.outs = [torch.empty(n, dtype=dt, device="cuda:0") for n, dt in shapes]
        self.want = {}

    def reset(self, stream):
        import torch

        with torch.cuda.stream(stream):
            for t in self.outs:
                t.fill_(0x5A)
            self.d_dg_work.copy_(self.d_dg)

    def run(self, stream, routes, neigh):
        e, o = self.eng, self.outs
        off = dict(n=N, offsets=self.d_dgoff, stream=stream)
        fr = dict(n=N, stride=P.FRAME_STRIDE, frame_len=P.FRAME_LEN, in_ifaces=self.d_ins, stream=stream)
        e.route_lookup_batch(routes, self.d_addrs, n=N, iface=o[0], next_hop=o[1], stream=stream)
        e.router_route_headers(routes, self.d_dg, hdrs=o[2], status=o[3], iface=o[4], next_hop=o[5], **off)
        e.router_route_batch(routes, self.d_dg_work, status=o[6], iface=o[7], next_hop=o[8], **off)
        e.frame_recv(neigh, self.d_frames, status=o[9], **fr)
        e.router_frames(routes, neigh, self.d_frames, hdrs=o[10], status=o[11], iface=o[12], next_hop=o[13], **fr)
        e.tcp_unwrap_batch(self.d_u, n=N, offsets=self.d_uoff, recs=o[14], status=None, stream=stream)
        e.tcp_unwrap_batch(self.d_u, n=N, offsets=self.d_uoff, recs=o[15], status=o[16], stream=stream)

    def results(self):
        return [t.clone() for t in self.outs] + [self.d_dg_work.clone()]

    def expected(self, router, rneigh):
        """the restatements' answers for every output, as numpy arrays in the outputs' order"""
        import test_gpu_frames as F

        rep = lambda a: np.tile(np.ascontiguousarray(a).reshape(P.K, -1), (5, 1)).reshape(-1)  # noqa: E731
        _, lf, lh = router.answers(self.addrs)
        st, fi, fh, hd, after = P.route_expect(self.dgrams, router)
        P.assert_route_classes(st)
        fst, ffi, ffh, frec = F.expect(self.frames, self.ins, router, rneigh)
        urec = P.unwrap_expect(self.unwraps)
        P.assert_unwrap_classes(urec, self.unwraps)
        return [rep(x) for x in (lf, lh, hd, st, fi, fh, st, fi, fh, fst & 0xF8, frec, fst, ffi, ffh, urec, urec,
                                 urec[:, 36])] + [np.tile(P.pack(after)[0], 5)], fst


def _as_np(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def test_threads_streams_and_tables(ceng):
    import torch
    from tcpip_network_protocol_stack_amd.engine import NeighTable, RouteTable

    rsets = [_routes_k(k) for k in range(TABLES)]
    routes = [fill(RouteTable(), r) for r in rsets]
    neighs = [_fill_neigh_k(NeighTable(), k) for k in range(TABLES)]
    routers = [RefRouter(r) for r in rsets]
    rneighs = [_fill_neigh_k(RefNeigh(), k) for k in range(TABLES)]
    jobs = [Job(ceng, t) for t in range(THREADS)]

    # serial results, each call alone on the default stream, compared in full with the restatements
    s0 = torch.cuda.current_stream()
    seen = []
    for t, j in enumerate(jobs):
        for k in PAIRS[t]:
            j.reset(s0)
            j.run(s0, routes[k], neighs[k])
            torch.cuda.synchronize()
            j.want[k] = j.results()
            want, fst = j.expected(routers[k], rneighs[k])
            seen.append(fst)
            for i, (g, w) in enumerate(zip(j.want[k], want)):
                assert np.array_equal(_as_np(g), w), (t, k, i)
    P.assert_frame_classes(np.concatenate(seen))

    errors = []
    start = threading.Barrier(THREADS)

    def body(job, tid):
        try:
            s = torch.cuda.Stream(device=0)
            start.wait(timeout=60)
            for r in range(ROUNDS):
                k = PAIRS[tid][r % 2]
                job.reset(s)
                job.run(s, routes[k], neighs[k])
                s.synchronize()
                for i, (g, w) in enumerate(zip(job.outs + [job.d_dg_work], job.want[k])):
                    if not torch.equal(g, w):
                        errors.append(f"thread {tid} round {r} tables {k} output {i} differs")
                        return
        except Exception as exc:  # surfaced by the assert below
            errors.append(f"thread {tid}: {exc!r}")

    threads = [threading.Thread(target=body, args=(j, t)) for t, j in enumerate(jobs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=100)
    assert not any(t.is_alive() for t in threads), "a worker thread did not finish"
    assert not errors, errors
    torch.cuda.synchronize()
    for t in routes + neighs:
        t.close()


# ----------------------------------------------------------------- A2 -----
ROUTE_ITEMS, ROUTE_CALLS = 1 << 24, 48
NEIGH_ITEMS, NEIGH_CALLS = 1 << 22, 24
S8, S32, SREC = 0x5A, 0x25A5A5A5, 0xA5


def _other_routes(routes, k):
    """the same prefixes, every interface and next hop another one: the image's structure stays"""
    return [(p, ln, f + 100 * k, has, (hop ^ (0x01010101 * k)) & 0xFFFFFFFF if has else 0) for p, ln, f, has, hop in routes]


def _other_neigh(t, k):
    import test_gpu_frames as F

    for f, ip in F.NEIGH:
        t.learn(f, ip, F._nmac(f, ip ^ (0x1100 * k)))
    return t


class RouteCase:
    """route_lookup_batch on the periodic addresses: T, the changed T and four tables of T's structure"""

    items, calls = ROUTE_ITEMS, ROUTE_CALLS

    def __init__(self, eng):
        import test_gpu_route as R
        from tcpip_network_protocol_stack_amd.engine import RouteTable

        self.eng, self.base = eng, R.ROUTES
        self.addrs = P.addr_items(R.ROUTES, 0xA2)
        self.table = fill(RouteTable(), R.ROUTES)
        self.others = [fill(RouteTable(), _other_routes(R.ROUTES, k)) for k in (2, 3, 4, 5)]
        for t in self.others:
            t.stats()  # compiled here, not on the timed path
        self.d_big = P.tile(_t(self.addrs), self.items)
        self.d_small = _t(self.addrs[:64])

    def want(self, k):
        """(iface, next_hop) over the K addresses for T (k = 0), the changed T (1), other table k"""
        _, f, h = RefRouter(self.base if k == 0 else _other_routes(self.base, k)).answers(self.addrs)
        return [f, h]

    def change(self):
        before = self.table.stats()
        fill(self.table, _other_routes(self.base, 1))
        after = self.table.stats()
        for key in ("route_records", "image_words", "l2_chunks", "l3_chunks"):
            assert before[key] == after[key], key

    def outputs(self, n):
        import torch

        return [P.sentinel(n, torch.int32, S32), P.sentinel(n, torch.int32, S32)]

    def call(self, table, big, outs, stream):
        self.eng.route_lookup_batch(table, self.d_big if big else self.d_small, n=self.items if big else 64,
                                    iface=outs[0][1], next_hop=outs[1][1], stream=stream)

    widths, sentinels = (1, 1), (S32, S32)

    def close(self):
        for t in [self.table] + self.others:
            t.close()


class NeighCase:
    """router_frames on the periodic frames: the neighbour table T, T with every address re-learnt, four more"""

    items, calls = NEIGH_ITEMS, NEIGH_CALLS

    def __init__(self, eng):
        import test_gpu_frames as F
        from tcpip_network_protocol_stack_amd.engine import NeighTable, RouteTable

        self.eng, self.F = eng, F
        self.frames, self.ins = P.frame_items(0xA3)
        self.routes = fill(RouteTable(), F.ROUTES)
        self.router = RefRouter(F.ROUTES)
        self.table = F._fill_neigh(NeighTable())
        self.others = [_other_neigh(F._fill_neigh(NeighTable()), k) for k in (2, 3, 4, 5)]
        for t in self.others:
            t.stats()  # compiled here, not on the timed path
        block = _t(P.frames_fixed(self.frames))
        self.d_big, self.d_big_ins = P.tile(block, self.items, P.FRAME_STRIDE), P.tile(_t(self.ins), self.items)
        self.d_small, self.d_small_ins = block[:64 * P.FRAME_STRIDE], _t(self.ins[:64])

    def want(self, k):
        ref = self.F._fill_neigh(RefNeigh())
        if k:
            _other_neigh(ref, k)
        st, fi, fh, rec = self.F.expect(self.frames, self.ins, self.router, ref)
        assert (st & 0x04).sum() > 100  # RESOLVED frames: their records carry the neighbour's address
        return [rec.reshape(-1), st, fi, fh]

    def change(self):
        before = self.table.stats()
        _other_neigh(self.table, 1)
        after = self.table.stats()
        for key in ("mappings", "image_ifaces", "image_slots"):
            assert before[key] == after[key], key

    def outputs(self, n):
        import torch

        return [P.sentinel(n * 36, torch.uint8, SREC), P.sentinel(n, torch.uint8, S8),
                P.sentinel(n, torch.int32, S32), P.sentinel(n, torch.int32, S32)]

    def call(self, table, big, outs, stream):
        n = self.items if big else 64
        self.eng.router_frames(self.routes, table, self.d_big if big else self.d_small, n=n, stride=P.FRAME_STRIDE,
                               frame_len=P.FRAME_LEN, in_ifaces=self.d_big_ins if big else self.d_small_ins,
                               hdrs=outs[0][1], status=outs[1][1], iface=outs[2][1], next_hop=outs[3][1],
                               stream=stream)

    widths, sentinels = (36, 1, 1, 1), (SREC, S8, S32, S32)

    def close(self):
        for t in [self.routes, self.table] + self.others:
            t.close()


def _check(case, outs, want, n, tag):
    """every output equals the K-item expectation repeated to n items, nothing written behind it"""
    import torch

    for i, ((whole, _), w, width, sent) in enumerate(zip(outs, want, case.widths, case.sentinels)):
        exp = P.tile(_t(w), n, width) if n > 64 else _t(w[:64 * width])
        got = whole[:n * width]
        if not torch.equal(got, exp):
            j = int((got != exp).nonzero()[0])
            raise AssertionError(f"{tag}: output {i} differs from item {j // width} on ({int(got[j]):#x}, want "
                                 f"{int(exp[j]):#x}; {int((got != exp).sum())} elements in all)")
        assert P.tail_untouched(whole, n * width, sent), (tag, i)


def _stream_beside(case, sa):
    """A stream whose launches run beside stream A's.  The runtime spreads its streams over a few hardware
    queues, and two streams on one queue run one behind the other: B's calls would then wait for A's whole
    queue and the case would test nothing.  Probe: eight of A's launches, one small call on the candidate;
    the candidate is done while A is still busy."""
    import torch

    big, small = case.outputs(case.items), case.outputs(64)
    for _ in range(6):
        sb = torch.cuda.Stream(device=0)
        torch.cuda.synchronize()
        for _ in range(8):
            case.call(case.table, True, big, sa)
        case.call(case.table, False, small, sb)
        sb.synchronize()
        beside = not sa.query()
        torch.cuda.synchronize()
        if beside:
            return sb
    raise AssertionError("no stream of six ran beside stream A")


@pytest.mark.parametrize("evict", [False, True], ids=["changed", "evicted"])
@pytest.mark.parametrize("kind", [RouteCase, NeighCase], ids=["route", "neigh"])
def test_image_is_not_replaced_under_another_streams_launch(ceng, kind, evict):
    import torch

    case = kind(ceng)
    old = case.want(0)
    sa = torch.cuda.Stream(device=0)
    sb = _stream_beside(case, sa)
    a_outs = [case.outputs(case.items) for _ in range(case.calls)]
    b1 = case.outputs(64)
    b_next = [case.outputs(64) for _ in range(4 if evict else 1)]
    warm = case.outputs(64)
    # Before A starts: the four other tables, then T, through the slots.  T's image is on the device, every
    # slot has its buffer (no allocation on the timed path), the slots hold others[1..3] and T, and T is the
    # most recently used: calls on others[1..3] hit, the call on others[0] then re-keys T's slot.
    for t in (case.others if evict else []) + [case.table]:
        case.call(t, False, warm, sb)
    torch.cuda.synchronize()
    order = [1, 2, 3, 0]
    for o in a_outs:                                   # 1
        case.call(case.table, True, o, sa)
    case.call(case.table, False, b1, sb)               # 2
    if evict:
        for i, o in zip(order, b_next):                # four tables through the slots: the last re-keys T's
            busy = not sa.query()
            case.call(case.others[i], False, o, sb)
    else:
        case.change()                                  # 3
        busy = not sa.query()
        case.call(case.table, False, b_next[0], sb)    # 4: uploads the new image
    torch.cuda.synchronize()                           # 5
    assert busy, "stream A had drained before the image was replaced: the case tested nothing"
    for j, o in enumerate(a_outs):
        _check(case, o, old, case.items, f"A's call {j} (old table)")
    _check(case, b1, old, 64, "B's first call (old table)")
    if evict:
        for i, o in zip(order, b_next):
            _check(case, o, case.want(i + 2), 64, f"B's call on other table {i}")
    else:
        _check(case, b_next[0], case.want(1), 64, "B's second call (new table)")
    case.close()
