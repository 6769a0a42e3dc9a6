"""CPU: the batches of tests/host_chunks.py reach what the GPU sweep of
tests/test_gpu_host_chunks.py claims to walk through the host-memory pipeline
(icsum_host.cpp), proven from the inputs alone: every chunk payload, chunk
start residue, empty-segment position, piece length and position, chunk count
per slot count, fixed-stride form and count cut is present, and every plan of
the model partitions the batch, stays within both caps and is maximal —
properties of the contract (greedy, maximal, a segment longer than a slot as
slot-sized pieces), checked here without the model's own arithmetic.  If a
generator is thinned below one of these conditions a test here fails; a
changed kSlotSegs, kWrapSlotSegs, kMaxSlots or kSubPiece moves the inputs
with it (they are read from the sources as text) or fails."""
import numpy as np
import pytest

import host_chunks as hc

S = hc.S


def _bounds(spec):
    if isinstance(spec, tuple):
        stride, seg_len = spec
        return lambda i: (i * stride, i * stride + seg_len)
    a = np.asarray(spec, dtype=np.uint64).astype(np.int64)
    return lambda i: (int(a[i]), int(a[i + 1]))


def check_plan(chunks, n, spec, slot, cap_n):
    """partition of [0, n), both caps, maximal; pieces tile their segment"""
    seg = _bounds(spec)
    nxt = k = 0
    while k < len(chunks):
        c = chunks[k]
        assert c.i0 == nxt, (k, c)
        s0, e0 = seg(c.i0)
        if c.piece:
            assert e0 - s0 > slot and c.i1 == c.i0 + 1, (k, c)
            pos = 0
            while True:
                c = chunks[k]
                assert c.piece and (c.i0, c.i1) == (nxt, nxt + 1) and c.pos == pos and c.b0 == s0 + pos, (k, c)
                assert 0 < c.b1 - c.b0 <= slot, (k, c)
                pos += c.b1 - c.b0
                k += 1
                assert c.last == (pos == e0 - s0), (k, c)
                if c.last:
                    break
                assert c.b1 - c.b0 == slot, (k, c)  # every piece but the last is a whole slot
            nxt += 1
            continue
        assert not c.last and c.pos == 0
        assert 0 < c.i1 - c.i0 <= cap_n and c.i1 <= n, (k, c)
        assert c.b0 == s0 and c.b1 == seg(c.i1 - 1)[1] and 0 <= c.b1 - c.b0 <= slot, (k, c)
        if c.i1 < n:  # one more segment would exceed a cap
            assert c.i1 - c.i0 == cap_n or seg(c.i1)[1] - c.b0 > slot, (k, c)
        nxt = c.i1
        k += 1
    assert nxt == n


# ---------------------------------------------------------- constants -----
def test_constants_read_from_the_sources():
    assert hc.K_SLOT_SEGS >= hc.K_WRAP_SLOT_SEGS > 16 and hc.K_SUB_PIECE % 2 == 0
    assert max(hc.NSLOTS) == hc.K_MAX_SLOTS and min(hc.NSLOTS) == 2
    assert S % hc.K_SUB_PIECE == 0 and S > 2 * hc.K_SUB_PIECE  # a whole piece is several sub-pieces
    # a chunk of cap tiny segments (mean < 0.5 byte) and the long one stays under a slot: the count cuts first
    assert hc.K_SLOT_SEGS * 0.5 + hc.LONG_SEG + 4 * 60 < S
    with pytest.raises(AssertionError):
        hc._const("icsum_ctx.h", "kNoSuchConstant")


# ----------------------------------------------------------- the model ----
def test_model_against_hand_cut_plans():
    C = hc.Chunk
    assert hc.plan(4, hc.offsets_of([3, 4, 3, 1]), 8, 10, False) == \
        [C(0, 2, 0, 7, False, 0, False), C(2, 4, 7, 11, False, 0, False)]
    assert hc.plan(4, hc.offsets_of([3, 4, 3, 1], 5), 8, 1, False) == \
        [C(i, i + 1, a, b, False, 0, False) for i, (a, b) in enumerate(((5, 8), (8, 12), (12, 15), (15, 16)))]
    assert hc.plan(3, hc.offsets_of([1, 17, 0]), 8, 10, True) == \
        [C(0, 1, 0, 1, False, 0, False), C(1, 2, 1, 9, True, 0, False), C(1, 2, 9, 17, True, 8, False),
         C(1, 2, 17, 18, True, 16, True), C(2, 3, 18, 18, False, 0, False)]
    with pytest.raises(ValueError):
        hc.plan(3, hc.offsets_of([1, 17, 0]), 8, 10, False)
    # fixed stride: k segments take (k - 1) stride + len bytes
    assert [(c.i0, c.i1, c.b0, c.b1) for c in hc.plan(5, (6, 2), 8, 10, False)] == \
        [(0, 2, 0, 8), (2, 4, 12, 20), (4, 5, 24, 26)]
    assert [(c.i0, c.i1, c.b0, c.b1) for c in hc.plan(9, (1, 5), 8, 10, False)] == [(0, 4, 0, 8), (4, 8, 4, 12), (8, 9, 8, 13)]
    assert [(c.i0, c.i1) for c in hc.plan(25, (0, 5), 8, 10, False)] == [(0, 10), (10, 20), (20, 25)]
    assert [(c.i0, c.i1, c.b0, c.b1) for c in hc.plan(3, (20, 8), 8, 10, False)] == [(0, 1, 0, 8), (1, 2, 20, 28), (2, 3, 40, 48)]
    assert hc.counters(hc.plan(2, (4, 4), 8, 10, False)) == (1, 0)
    assert hc.counters(hc.plan(3, (4, 4), 8, 10, False)) == (0, 2)
    assert hc.counters(hc.plan(1, (9, 9), 8, 10, True)) == (0, 2)
    assert hc.counters(hc.plan(1, (4, 4), 8, 10, False), zero_copy_max=3) == (0, 1)


def test_checker_rejects_plans_that_break_the_contract():
    off = hc.offsets_of([3, 4, 3, 1])
    good = hc.plan(4, off, 8, 10, False)
    check_plan(good, 4, off, 8, 10)
    C = hc.Chunk
    for bad in ([good[0]],  # no partition
                [C(0, 1, 0, 3, False, 0, False), C(1, 4, 3, 11, False, 0, False)],  # not maximal
                [C(0, 3, 0, 10, False, 0, False), C(3, 4, 10, 11, False, 0, False)]):  # over the byte cap
        with pytest.raises(AssertionError):
            check_plan(bad, 4, off, 8, 10)
    with pytest.raises(AssertionError):  # over the count cap
        check_plan(good, 4, off, 8, 1)


# --------------------------------------------------- offsets batches ------
@pytest.fixture(scope="module")
def cuts():
    out = []
    for name, lens in hc.cut_batches():
        off = hc.offsets_of(lens)
        out.append((name, lens, off, hc.plan(lens.size, off, S, hc.K_SLOT_SEGS, False)))
    return out


def test_cut_batches_reach_every_class(cuts):
    cls = [hc.chunk_classes(lens, p) for _, lens, _, p in cuts]
    pay = set().union(*(c["payloads"] for c in cls))
    assert {0, 1} <= pay and any(c["plus_one"] for c in cls)  # S, S - 1, and S + 1 refused
    assert set().union(*(c["residues"] for c in cls)) == set(range(16))
    for key in ("empty_first", "empty_last", "empty_tail"):
        assert any(c[key] for c in cls), key
    want = {k for s in hc.NSLOTS for k in (1, s - 1, s, s + 1, 2 * s + 1)}
    assert {c["count"] for c in cls} == want
    assert any((lens == S).any() for _, lens, _, _ in cuts)  # a segment of one slot exactly
    assert all(lens.max() <= S for _, lens, _, _ in cuts)  # every entry point takes them
    # the chunks' mean lengths reach the tiny kernel's range and the long-segment shapes
    means = [(c.b1 - c.b0) / (c.i1 - c.i0) for _, _, _, p in cuts for c in p]
    assert min(means) < 64 and max(means) == S and any(500 < x < 3000 for x in means)
    assert sum(int(lens.sum()) for _, lens, _, _ in cuts) < 32 << 20


def test_thinned_cut_batches_would_be_noticed(cuts):
    # without the nine-chunk batch: 2 x 4 + 1 chunks and some start residues go missing
    cls = [hc.chunk_classes(lens, p) for name, lens, _, p in cuts if name != "cut9"]
    assert 9 not in {c["count"] for c in cls}
    assert set().union(*(c["residues"] for c in cls)) != set(range(16))
    # a plan under a larger slot has no cut where these batches put theirs
    name, lens, off, p = cuts[-1]
    assert len(hc.plan(lens.size, off, 2 * S, hc.K_SLOT_SEGS, False)) < len(p)


def test_piece_batches_reach_every_class():
    cls = []
    lens_all = []
    for _, lens in hc.piece_batches():
        off = hc.offsets_of(lens)
        p = hc.plan(lens.size, off, S, hc.K_SLOT_SEGS, True)
        check_plan(p, lens.size, off, S, hc.K_SLOT_SEGS)
        with pytest.raises(ValueError):
            hc.plan(lens.size, off, S, hc.K_SLOT_SEGS, False)
        cls.append(hc.chunk_classes(lens, p))
        lens_all += lens.tolist()
    assert {S + 1, 2 * S, 2 * S + 1, 3 * S - 1} <= set(lens_all)
    tails = set().union(*(c["piece_tails"] for c in cls))
    assert {1, hc.K_SUB_PIECE - 1, hc.K_SUB_PIECE, hc.K_SUB_PIECE + 1, S, S - 1} <= tails
    assert set().union(*(c["piece_at"] for c in cls)) == {"first", "middle", "last", "adjacent"}
    assert any(c["empty_chunk"] for c in cls)  # an empty segment between two pieced ones: a chunk of no bytes
    # pieced segments start at odd and at even offsets
    par = {int(hc.offsets_of(lens)[i]) & 1 for _, lens in hc.piece_batches() for i in np.flatnonzero(lens > S)}
    assert par == {0, 1}


def test_every_offsets_plan_keeps_the_contract(cuts):
    for name, lens, off, p in cuts:
        check_plan(p, lens.size, off, S, hc.K_SLOT_SEGS)
        check_plan(hc.plan(lens.size, off, S, hc.K_WRAP_SLOT_SEGS, False), lens.size, off, S, hc.K_WRAP_SLOT_SEGS)
        lead = hc.offsets_of(lens, 3)  # the plan does not depend on the lead
        assert [(c.i0, c.i1) for c in hc.plan(lens.size, lead, S, hc.K_SLOT_SEGS, False)] == [(c.i0, c.i1) for c in p], name


# ------------------------------------------------------- fixed stride -----
def test_fixed_batches_name_every_form():
    f = [(st, ln) for _, st, ln, _, _ in hc.FIXED]
    assert any(st == ln > 0 for st, ln in f) and any(st > ln > 0 for st, ln in f)
    assert any(1 < st < ln for st, ln in f) and any(st == 1 < ln for st, ln in f)
    assert any(st == 0 < ln for st, ln in f) and any(st > S >= ln > 0 for st, ln in f)
    assert any(st > S and ln == S for st, ln in f)
    assert any(ln == 0 < st for st, ln in f) and (0, 0) in f
    assert all(ln <= S for st, ln in f)
    assert all(ln > S for _, _, ln, _, _ in hc.FIXED_PIECES)
    assert any(st < ln for _, st, ln, _, _ in hc.FIXED_PIECES) and any(st >= ln for _, st, ln, _, _ in hc.FIXED_PIECES)
    for _, st, ln, n, overlapping in hc.FIXED + hc.FIXED_PIECES:
        assert overlapping == (n > 1 and st < ln) or ln == 0
        assert hc.fixed_bytes(st, ln, n) < 8 << 20


def test_every_fixed_plan_keeps_the_contract():
    counts = {}
    for name, st, ln, n, _ in hc.FIXED + hc.FIXED_PIECES:
        for cap in (hc.K_SLOT_SEGS, hc.K_WRAP_SLOT_SEGS):
            p = hc.plan(n, (st, ln), S, cap, ln > S)
            check_plan(p, n, (st, ln), S, cap)
            assert p[-1].b1 == hc.fixed_bytes(st, ln, n)
        counts[name] = len(p)
    # several chunks where the form allows it at these sizes; the padding behind
    # a chunk's last segment and overlapping neighbours do not count
    assert counts["stride_eq_len"] == 3 and counts["stride_gt_len"] == 3 and counts["stride_lt_len"] == 3
    assert counts["stride_1"] == counts["stride_0"] == counts["len_0_stride_7"] == counts["len_0_stride_0"] == 1
    assert counts["stride_gt_slot"] == 5 and counts["stride_gt_slot_len_eq_slot"] == 3 and counts["len_0"] == 3
    p = hc.plan(600, (4096, 0), S, hc.K_SLOT_SEGS, False)
    assert p[0].b1 - p[0].b0 == S  # a chunk of S bytes exactly and no segment bytes
    p = hc.plan(4000, (600, 100), S, hc.K_SLOT_SEGS, False)
    assert (p[0].i1 - 1) * 600 + 100 <= S < p[0].i1 * 600  # the last segment fits, its padding would not


# --------------------------------------------------------- count cuts -----
@pytest.mark.parametrize("cap,ds", [(hc.K_SLOT_SEGS, (0, 1, 3)), (hc.K_WRAP_SLOT_SEGS, (0, 1))],
                         ids=["kSlotSegs", "kWrapSlotSegs"])
def test_count_cut_batches(cap, ds):
    for d in ds:
        lens, valid = hc.count_cut_batch(cap, d, 77 + d)
        n = lens.size
        assert n == 2 * cap + d and lens.max() == hc.LONG_SEG
        core = lens[cap:]
        assert set(np.unique(np.delete(core, np.concatenate([[cap // 3], valid - cap]))).tolist()) == {0, 1, 2}
        off = hc.offsets_of(lens)
        p = hc.plan(n, off, S, cap, False)
        check_plan(p, n, off, S, cap)
        assert [(c.i0, c.i1) for c in p] == [(0, cap), (cap, 2 * cap)] + ([(2 * cap, n)] if d else [])
        assert p[0].b1 == p[0].b0  # a whole chunk of empty segments
        # the count decides both cuts: the bytes would have let the next segment in
        for c in p[:-1]:
            assert c.i1 - c.i0 == cap and int(off[c.i1 + 1]) - c.b0 <= S
        assert p[-1].i1 - p[-1].i0 == (d or cap)
        # the long segment sits in a chunk whose mean length is below 2 bytes
        assert cap < cap + cap // 3 < 2 * cap and (p[1].b1 - p[1].b0) / cap < 2
        # valid 40..60-byte datagrams on either side of each cut
        assert {cap, 2 * cap - 1} <= set(valid.tolist()) and (d == 0 or 2 * cap in valid)
        assert all(40 <= lens[i] <= 60 for i in valid)
        # and without the count cap the plan would differ: the cap is what these batches test
        assert len(hc.plan(n, off, S, 4 * cap, False)) == 1


# ------------------------------------------------------ the wire, vectorised
def test_vectorised_wire_equals_the_per_datagram_oracle(orc):
    from helpers import pack_contiguous
    from test_gpu_wrap import _oracle_wire, _random_batch

    rng = np.random.default_rng(3)
    segs, m = _random_batch(rng, 300)
    segs[5] = b"\0" * 40 + rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()  # the length field wraps
    segs[7], segs[8], segs[9] = b"\x5a" * 39, b"\x45" * 25, b""  # shorter than 40: untouched
    want = _oracle_wire(orc, segs[:7], m[:7]) + segs[7:10] + _oracle_wire(orc, segs[10:], m[10:])
    buf, off = pack_contiguous(segs, 3)
    got = hc.wire_in_place(orc, buf, m, offsets=off)
    for i, w in enumerate(want):
        assert got[off[i]:off[i + 1]].tobytes() == w, i
    assert (got[:3] == buf[:3]).all() and (got[int(off[-1]):] == buf[int(off[-1]):]).all()
    keep = [i for i in range(300) if i not in (7, 8, 9)]
    pb, poff = pack_contiguous([segs[i][40:] for i in keep], 2)
    hdrs = hc.wire_headers(orc, pb, m[keep], offsets=poff)
    for j, i in enumerate(keep):
        assert hdrs[40 * j:40 * j + 40].tobytes() == want[i][:40], i
    # fixed stride
    L = 104
    _, m2 = _random_batch(rng, 50, fixed=L - 40)
    body = rng.integers(0, 256, 50 * L, dtype=np.uint8)
    got = hc.wire_in_place(orc, body, m2, stride=L, dgram_len=L)
    hd = hc.wire_headers(orc, body, m2, stride=L, payload_len=L - 40)
    for i in range(50):
        w = _oracle_wire(orc, [b"\0" * 40 + body[i * L + 40:(i + 1) * L].tobytes()], m2[i:i + 1])[0]
        assert got[i * L:(i + 1) * L].tobytes() == w, i
        w = _oracle_wire(orc, [b"\0" * 40 + body[i * L:i * L + L - 40].tobytes()], m2[i:i + 1])[0]
        assert hd[40 * i:40 * i + 40].tobytes() == w[:40], i


def test_fill_dresses_datagrams():
    rng = np.random.default_rng(4)
    lens = np.array([0, 19, 20, 45, 3000, 1, 60])
    buf = hc.fill(rng, lens, valid=(3, 6))
    off = hc.offsets_of(lens).astype(np.int64)
    assert buf.size == lens.sum() and all(buf[off[i]] >> 4 == 4 for i in (2, 3, 4, 6))
    assert buf[off[3]] == 0x45 and (buf[off[3] + 2] << 8 | buf[off[3] + 3]) == 45 and buf[off[3] + 9] == 6
    init = hc.inits_for(rng, 7)
    assert {0, 0xFFFFFFFF} <= set(init.tolist()) and hc.inits_for(rng, 1).size == 1
