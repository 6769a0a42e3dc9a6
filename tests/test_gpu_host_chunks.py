"""GPU: the host-memory pipeline (icsum_host.cpp) walked through its chunk
cuts, slot turns and pieces.

Engines with 1 MiB staging slots and 2, 3 and 4 of them (and the
bounds-checked build) take the batches of tests/host_chunks.py — chunk
payloads of S - 1 and S bytes and a refused S + 1, chunk starts at every
residue mod 16, empty segments first, last and trailing, segments of one slot
exactly and of pieces with 1-byte and sub-piece-edge tails, every fixed-stride
form, and the count cuts at kSlotSegs and kWrapSlotSegs — from pageable and
page-locked memory at buffer leads 0 and 3: checksum with inits, the fused
IPv4 kernel in COMPUTE, VERIFY and PATCH, the in-place and the headers-apart
wrap, each against the oracle, the whole caller buffer compared afterwards,
outputs passed in filled with a sentinel and guard elements past n, and the
chunk counters of ics_dispatch_info equal to the model's plan
(tests/test_host_chunks.py proves what the batches reach)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import host_chunks as hc

pytestmark = pytest.mark.gpu

S, G = hc.S, hc.GUARD
SENT16, SENT8 = 0xA5C3, 0xA5


def _engine(env, debug=False):
    """engine_with() under these environment variables (read at ics_create), restored after"""
    from conftest import engine_with

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        gen = engine_with(debug=debug)
        eng = next(gen)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return gen, eng


@pytest.fixture(scope="module", params=[(2, False), (3, False), (4, False), (3, True)],
                ids=["slots2", "slots3", "slots4", "slots3-bounds"])
def ceng(request):
    slots, debug = request.param
    gen, eng = _engine({"ICSUM_HOST_SLOT_MB": str(hc.SLOT_MB), "ICSUM_HOST_SLOTS": str(slots)}, debug)
    yield eng
    next(gen, None)


# -------------------------------------------------- references, computed once
_CASES = {}


def _case(orc, name, build):
    if name not in _CASES:
        _CASES[name] = build()
        for v in vars(_CASES[name]).values():  # shared among the tests: left unchanged
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _CASES[name]


def _offsets_case(orc, name, lens, valid=(), seed=1, kinds="cipw", wrap_cap=hc.K_WRAP_SLOT_SEGS):
    """kinds: c checksum, i the fused IPv4 kernel, w both wraps"""
    def build():
        rng = np.random.default_rng(seed)
        n = lens.size
        off = hc.offsets_of(lens)
        c = SimpleNamespace(name=name, lens=lens, n=n, data=hc.fill(rng, lens, valid), init=hc.inits_for(rng, n))
        c.ck = orc.checksum_batch(c.data, n, offsets=off, init=c.init)
        c.plan_ck = hc.counters(hc.plan(n, off, S, hc.K_SLOT_SEGS, True))
        if "i" in kinds:
            c.ipv4 = []
            for mode in (0, 1, 2):
                after = c.data.copy()
                c.ipv4.append(orc.ipv4_tcp_batch(after, n, mode, offsets=off) + (after,))
            assert (c.ipv4[0][3] == c.data).all() and (c.ipv4[1][3] == c.data).all()
            c.plan_ip = hc.counters(hc.plan(n, off, S, hc.K_SLOT_SEGS, False))
        if "w" in kinds:
            c.msgs = hc.random_msgs(rng, n)
            c.wire = hc.wire_in_place(orc, c.data, c.msgs, offsets=off)
            c.hdrs = hc.wire_headers(orc, c.data, c.msgs, offsets=off)
            c.plan_wrap = hc.counters(hc.plan(n, off, S, wrap_cap, False))
        return c
    return _case(orc, name, build)


def _host(data, lead, pinned):
    """`data` behind `lead` bytes of a fresh allocation, 16 guard bytes behind it"""
    import torch

    h = torch.empty(lead + data.size + 16, dtype=torch.uint8, pin_memory=pinned).numpy()
    h[:lead] = SENT8
    h[lead:lead + data.size] = data
    h[lead + data.size:] = SENT8
    return h


def _same(h, want, lead, what):
    body = h[lead:lead + want.size]
    if not np.array_equal(body, want):
        bad = np.flatnonzero(body != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ, first at {bad[:5].tolist()}")
    assert (h[:lead] == SENT8).all() and (h[lead + want.size:] == SENT8).all(), what


def _eq(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[:5].tolist()}: "
                             f"got {got[bad[:5]].tolist()} want {want[bad[:5]].tolist()}")


def _counted(eng, want, what, call):
    a = eng.dispatch_info()
    r = call()
    b = eng.dispatch_info()
    got = (b["host_zero_copy"] - a["host_zero_copy"], b["host_dma_chunks"] - a["host_dma_chunks"])
    assert got == want, f"{what}: (zero-copy calls, DMA'd chunks) {got}, the model's plan has {want}"
    return r


def _outs(n):
    return (np.full(n + G, SENT16, dtype=np.uint16), np.full(n + G, SENT16 ^ 0x1111, dtype=np.uint16),
            np.full(n + G, SENT8, dtype=np.uint8))


def _run(eng, c, pinned, lead, off=None, stride=0, seg_len=0, kinds="cipw", writers=True):
    """every entry point of `kinds` over one case, offsets (from `lead`) or fixed stride"""
    n = c.n
    kw = {"offsets": off} if off is not None else {"stride": stride}
    tag = f"{c.name} lead {lead} pinned {pinned}"
    h = _host(c.data, lead, pinned)
    base = h if off is not None else h[lead:]
    if "c" in kinds:
        out, _, _ = _outs(n)
        _counted(eng, c.plan_ck, tag + " checksum",
                 lambda: eng.checksum_batch_host(base, n, init=c.init, out=out, seg_len=seg_len, **kw))
        _eq(out[:n], c.ck, tag + " checksum")
        assert (out[n:] == SENT16).all(), tag
        _same(h, c.data, lead, tag + " checksum")
    if "i" in kinds:
        for mode in (0, 1, 2) if writers else (0, 1):
            ip, tcp, st = _outs(n)
            _counted(eng, c.plan_ip, f"{tag} ipv4 mode {mode}",
                     lambda: eng.ipv4_tcp_batch_host(base, n, mode, dgram_len=seg_len, ip_ck=ip, tcp_ck=tcp,
                                                     status=st, **kw))
            w = c.ipv4[mode]
            _eq(ip[:n], w[0], f"{tag} mode {mode} ip_ck")
            _eq(tcp[:n], w[1], f"{tag} mode {mode} tcp_ck")
            _eq(st[:n], w[2], f"{tag} mode {mode} status")
            assert (ip[n:] == SENT16).all() and (tcp[n:] == SENT16 ^ 0x1111).all() and (st[n:] == SENT8).all(), tag
            _same(h, w[3], lead, f"{tag} mode {mode}")
    if "w" in kinds:
        if writers:
            h = _host(c.data, lead, pinned)
            base = h if off is not None else h[lead:]
            _counted(eng, c.plan_wrap, tag + " wrap in place",
                     lambda: eng.tcp_wrap_batch_host(base, c.msgs, n, dgram_len=seg_len, **kw))
            _same(h, c.wire, lead, tag + " wrap in place")
        h = _host(c.data, lead, pinned)
        base = h if off is not None else h[lead:]
        hdrs = np.full(40 * n + G, SENT8, dtype=np.uint8)
        _counted(eng, c.plan_wrap, tag + " wrap headers apart",
                 lambda: eng.tcp_wrap_headers_host(base, c.msgs, n, payload_len=seg_len, hdrs=hdrs, **kw))
        _eq(hdrs[:40 * n], c.hdrs, tag + " wrap headers apart")
        assert (hdrs[40 * n:] == SENT8).all(), tag
        _same(h, c.data, lead, tag + " wrap headers apart")


MEM = pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
LEAD = pytest.mark.parametrize("lead", [0, 3])


# ------------------------------------------------------------- the sweeps --
@MEM
@LEAD
def test_byte_cuts_every_entry_point(ceng, orc, pinned, lead):
    """chunk counts of 1, nslots - 1, nslots, nslots + 1 and 2 nslots + 1 for
    every slot count; payloads of S - 1, S and a refused S + 1; chunk starts at
    every residue mod 16 (the staged copy starts at residue 0); segments of S
    bytes; empty segments first, last and trailing"""
    for j, (name, lens) in enumerate(hc.cut_batches()):
        c = _offsets_case(orc, name, lens, seed=100 + j)
        _run(ceng, c, pinned, lead, off=hc.offsets_of(lens, lead))


@MEM
@LEAD
def test_pieces_checksum(ceng, orc, pinned, lead):
    """segments of S + 1, 2 S, 2 S + 1 and 3 S - 1 bytes and with last pieces
    of kSubPiece - 1, kSubPiece and kSubPiece + 1 bytes, first, in the middle,
    last and two adjacent (the running piece sum starts again at each), an
    empty segment between two of them, inits 0 and 0xFFFFFFFF"""
    for j, (name, lens) in enumerate(hc.piece_batches()):
        c = _offsets_case(orc, name, lens, seed=200 + j, kinds="c")
        _run(ceng, c, pinned, lead, off=hc.offsets_of(lens, lead), kinds="c")


def _fixed_case(orc, name, stride, seg_len, n, overlapping, seed):
    def build():
        rng = np.random.default_rng(seed)
        size = hc.fixed_bytes(stride, seg_len, n)
        data = rng.integers(0, 256, size, dtype=np.uint8)
        if seg_len >= 20 and stride:
            data[np.arange(n, dtype=np.int64) * stride] = 0x40 | rng.integers(0, 16, n).astype(np.uint8)
        c = SimpleNamespace(name=name, n=n, data=data, init=hc.inits_for(rng, n))
        c.ck = orc.checksum_batch(data, n, stride=stride, seg_len=seg_len, init=c.init)
        pieces = seg_len > S
        c.plan_ck = hc.counters(hc.plan(n, (stride, seg_len), S, hc.K_SLOT_SEGS, pieces))
        if pieces:
            return c
        c.ipv4 = []
        for mode in (0, 1) if overlapping else (0, 1, 2):
            after = data.copy()
            c.ipv4.append(orc.ipv4_tcp_batch(after, n, mode, stride=stride, dgram_len=seg_len) + (after,))
        c.plan_ip = hc.counters(hc.plan(n, (stride, seg_len), S, hc.K_SLOT_SEGS, False))
        c.msgs = hc.random_msgs(rng, n)
        if not overlapping:
            c.wire = hc.wire_in_place(orc, data, c.msgs, stride=stride, dgram_len=seg_len)
        c.hdrs = hc.wire_headers(orc, data, c.msgs, stride=stride, payload_len=seg_len)
        c.plan_wrap = hc.counters(hc.plan(n, (stride, seg_len), S, hc.K_WRAP_SLOT_SEGS, False))
        return c
    return _case(orc, name, build)


@MEM
@LEAD
def test_fixed_stride_forms(ceng, orc, pinned, lead):
    """stride = len, > len, < len (64 and 1), 0, > S with len <= S and len =
    S, len 0 (chunks of S bytes and no segment bytes), and len > S through the
    checksum's pieces; overlapping batches through what only reads"""
    for j, (name, stride, seg_len, n, overlapping) in enumerate(hc.FIXED + hc.FIXED_PIECES):
        c = _fixed_case(orc, name, stride, seg_len, n, overlapping, 300 + j)
        _run(ceng, c, pinned, lead, stride=stride, seg_len=seg_len, kinds="c" if seg_len > S else "cipw",
             writers=not overlapping)


@MEM
@LEAD
@pytest.mark.parametrize("d", [0, 1, 3])
def test_count_cut_checksum_and_ipv4(ceng, orc, pinned, lead, d):
    """2 kSlotSegs + d segments: a chunk of kSlotSegs empty segments (no
    bytes), a chunk of kSlotSegs segments of 0..2 bytes holding one 300 KB
    segment (cut by count with bytes to spare), d segments behind it; valid
    datagrams on either side of each cut"""
    lens, valid = hc.count_cut_batch(hc.K_SLOT_SEGS, d, 77 + d)
    c = _offsets_case(orc, f"count{d}", lens, valid, seed=400 + d, kinds="ci")
    assert c.plan_ck == c.plan_ip == (0, 3 if d else 2)
    _run(ceng, c, pinned, lead, off=hc.offsets_of(lens, lead), kinds="ci")


@MEM
@LEAD
@pytest.mark.parametrize("d", [0, 1])
def test_count_cut_wraps(ceng, orc, pinned, lead, d):
    """the same at 2 kWrapSlotSegs + d records, in place (the 40..60-byte and
    the 300 KB datagrams get headers, the rest keep their bytes) and headers
    apart (every segment a payload)"""
    lens, valid = hc.count_cut_batch(hc.K_WRAP_SLOT_SEGS, d, 87 + d)
    c = _offsets_case(orc, f"wrapcount{d}", lens, valid, seed=500 + d, kinds="w")
    assert c.plan_wrap == (0, 3 if d else 2)
    _run(ceng, c, pinned, lead, off=hc.offsets_of(lens, lead), kinds="w")


# -------------------------------------------------------------- errors ----
def _clean(eng, orc):
    name, lens = hc.cut_batches()[2]
    c = _offsets_case(orc, name, lens, seed=102)
    _run(eng, c, False, 3, off=hc.offsets_of(lens, 3), kinds="ci", writers=False)


def test_offsets_not_monotone_at_every_position(ceng, orc):
    """a decreasing pair at index 0, inside a chunk, on a cut with
    offsets[i1 + 1] below the chunk's first offset (the cut's subtraction
    wraps), and at the last index: ICS_ERR_INVALID naming the pair, from every
    entry point, and the engine's next batch is exact"""
    from tcpip_network_protocol_stack_amd._lib import IcsumError

    name, lens = hc.cut_batches()[4]
    c = _offsets_case(orc, name, lens, seed=104)
    good = hc.offsets_of(lens, 3)
    p = hc.plan(c.n, good, S, hc.K_SLOT_SEGS, False)
    q = max(p[1:-1], key=lambda ch: ch.i1 - ch.i0)  # a chunk with chunks in flight before it and a cut behind it
    assert len(p) >= 4 and q.i1 - q.i0 > 20 and good[q.i0 + 9] > q.b0
    spots = {"first": (0, int(good[0]) - 1), "inside": (q.i0 + 9, None), "cut": (q.i1, q.b0 - 1),
             "last": (c.n - 1, None)}
    for what, (i, v) in spots.items():
        off = good.copy()
        off[i + 1] = int(off[i]) - 1 if v is None else v
        assert off[i + 1] < off[i] and (what != "cut" or off[i + 1] < q.b0)
        match = rf"not monotone: offsets\[{i}\] > offsets\[{i + 1}\]"
        h = _host(c.data, 3, False)
        with pytest.raises(IcsumError, match=match):
            ceng.checksum_batch_host(h, c.n, offsets=off, init=c.init)
        with pytest.raises(IcsumError, match=match):
            ceng.ipv4_tcp_batch_host(h, c.n, 1, offsets=off)
        with pytest.raises(IcsumError, match=match):
            ceng.tcp_wrap_headers_host(h, c.msgs, c.n, offsets=off)
        with pytest.raises(IcsumError, match=match):
            ceng.tcp_wrap_batch_host(h, c.msgs, c.n, offsets=off)
        _clean(ceng, orc)


def test_oversized_datagram_in_the_wraps(ceng, orc):
    """a datagram of S + 8 bytes (the wraps never split one) first, and behind
    four chunks already in flight: ICS_ERR_INVALID naming it, then exact"""
    from tcpip_network_protocol_stack_amd._lib import IcsumError

    name, lens = hc.cut_batches()[3]
    c = _offsets_case(orc, name, lens, seed=103)
    rng = np.random.default_rng(9)
    big = rng.integers(0, 256, S + 8, dtype=np.uint8)
    for what, ls, data, at in (("first", np.concatenate([[S + 8], lens]), np.concatenate([big, c.data]), 0),
                               ("late", np.concatenate([lens, [S + 8]]), np.concatenate([c.data, big]), c.n)):
        off = hc.offsets_of(ls, 1)
        m = np.resize(c.msgs, c.n + 1)
        match = rf"datagram {at} \({S + 8} bytes\) exceeds"
        for pinned in (False, True):
            h = _host(data, 1, pinned)
            with pytest.raises(IcsumError, match=match):
                ceng.tcp_wrap_batch_host(h, m, c.n + 1, offsets=off)
            with pytest.raises(IcsumError, match=match):
                ceng.tcp_wrap_headers_host(h, m, c.n + 1, offsets=off)
            del h
        _clean(ceng, orc)


# ------------------------------------------- the default 32 MiB engine ----
def test_threaded_retire_stores_equal_serial(orc):
    """70 000 x 64-byte datagrams are one DMA'd chunk of the default engine
    and four ranges of its retire stores (16 384 datagrams each at least):
    PATCH's fields and the in-place wrap's headers, fixed stride and offsets,
    with the copy workers at their default, at 1 (serial) and at 3 — the same
    bytes, the oracle's"""
    n, L = 70_000, 64
    rng = np.random.default_rng(0x70)
    data = rng.integers(0, 256, n * L, dtype=np.uint8)
    data[::L] = 0x40 | rng.integers(0, 16, n).astype(np.uint8)
    data[9::2 * L] = 6
    msgs = hc.random_msgs(rng, n)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    patched = data.copy()
    want = orc.ipv4_tcp_batch(patched, n, 2, stride=L, dgram_len=L)
    wire = hc.wire_in_place(orc, data, msgs, stride=L, dgram_len=L)
    assert (patched != data).any() and (wire != data).any()
    for threads in (None, "1", "3"):
        gen, eng = _engine({} if threads is None else {"ICSUM_COPY_THREADS": threads})
        try:
            for kw in ({"stride": L, "dgram_len": L}, {"offsets": off}):
                h = _host(data, 0, False)
                ip, tcp, st = _outs(n)
                _counted(eng, (0, 1), f"PATCH threads {threads}",
                         lambda: eng.ipv4_tcp_batch_host(h, n, 2, ip_ck=ip, tcp_ck=tcp, status=st, **kw))
                _eq(ip[:n], want[0], f"threads {threads} ip_ck")
                _eq(tcp[:n], want[1], f"threads {threads} tcp_ck")
                _eq(st[:n], want[2], f"threads {threads} status")
                _same(h, patched, 0, f"PATCH threads {threads} {sorted(kw)}")
                h = _host(data, 0, False)
                _counted(eng, (0, 1), f"wrap threads {threads}", lambda: eng.tcp_wrap_batch_host(h, msgs, n, **kw))
                _same(h, wire, 0, f"wrap in place threads {threads} {sorted(kw)}")
        finally:
            next(gen, None)


def test_staging_copy_split_from_an_odd_address(engine, orc):
    """a pageable batch of 9 MiB + 5 bytes starting one byte into its
    allocation: one chunk of the default engine, its staging copy split over
    two workers (4 MiB each at least)"""
    rng = np.random.default_rng(0x9)
    total = (9 << 20) + 5
    lens = rng.integers(0, 3000, 6200)
    lens = np.concatenate([lens, [total - int(lens.sum())]])
    assert lens[-1] >= 0
    n = lens.size
    alloc = np.empty(total + 1 + 16, dtype=np.uint8)
    h = alloc[1 - alloc.ctypes.data % 2:]
    assert h.ctypes.data % 2 == 1
    data = rng.integers(0, 256, total, dtype=np.uint8)
    h[:total] = data
    h[total:] = SENT8
    off = hc.offsets_of(lens)
    init = hc.inits_for(rng, n)
    out, _, _ = _outs(n)
    _counted(engine, (0, 1), "9 MiB + 5", lambda: engine.checksum_batch_host(h, n, offsets=off, init=init, out=out))
    _eq(out[:n], orc.checksum_batch(data, n, offsets=off, init=init), "9 MiB + 5 checksum")
    assert (out[n:] == SENT16).all() and (h[:total] == data).all() and (h[total:] == SENT8).all()
