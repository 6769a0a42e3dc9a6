"""CPU: the coverage claims of lattice_headers.py and periodic.py, proven from
the inputs alone (no GPU, no library): what test_gpu_frames' and
test_gpu_unwrap's lattice cases, test_gpu_grid_stride.py and
test_gpu_concurrency_tables.py rely on."""
import numpy as np

import lattice_headers as LH
import periodic as P
from frame_ref import RefNeigh
from route_ref import RefRouter


def _hop_refs():
    import test_gpu_frames as F

    return RefRouter(F.ROUTES), F._fill_neigh(RefNeigh())


def _starts(off, which):
    """{target: (start, length)} of one batch"""
    return {int(t): (int(off[i]), int(off[i + 1] - off[i])) for i, t in enumerate(which) if t >= 0}


def test_frame_lattice_classes():
    frames, ins, res = LH.frame_targets()
    assert sorted({len(f) for f in frames}) == LH.FRAME_LENGTHS
    assert {(len(f), int(r)) for f, r in zip(frames, res)} == {(L, r) for L in LH.FRAME_LENGTHS for r in range(16)}
    nb = LH.n_batches(len(frames))
    assert nb == 80
    last, held = set(), set()
    for b in range(nb):
        items, off, which = LH.batch(frames, res, b, seed=1)
        at = _starts(off, which)
        assert sorted(at) == list(range(len(frames)))  # every target in every batch
        for t, (s, ln) in at.items():
            assert s % 16 == res[t] and ln == len(frames[t])
            # (blocks held capped at the four the kernel loads, whether the load clamps at the last block)
            held.add((min(LH.blocks_held(s, ln), 4), LH.blocks_held(s, ln) < 4))
        assert all(len(x) < 16 for x, t in zip(items, which) if t < 0)  # a pad never holds a datagram
        assert which[-1] == 3 * b and int(off[-1]) == sum(len(x) for x in items)  # it ends the allocation
        last.add(int(which[-1]))
    assert len(last) == nb and 3 * len(last) >= len(frames)
    assert held == {(1, True), (2, True), (3, True), (4, False)}
    # every length class ends an allocation, at several residues
    assert {len(frames[t]) for t in last} == set(LH.FRAME_LENGTHS)
    assert len({int(res[t]) for t in last}) == 16


def test_frame_lattice_status_classes():
    import test_gpu_frames as F

    frames, ins, _ = LH.frame_targets()
    router, rneigh = _hop_refs()
    st, _, _, _ = F.expect(frames, ins, router, rneigh)
    P.assert_frame_classes(st)
    # ... and per length class what can exist there exists
    by_len = {L: st[[i for i, f in enumerate(frames) if len(f) == L]] for L in LH.FRAME_LENGTHS}
    assert (by_len[13] == 0).all()
    for L in (14, 15, 29, 30, 33):
        assert (by_len[L] & F.FR_DGRAM == 0).all() and (by_len[L] & F.FR_FOR_US != 0).any()
    for L in (34, 35, 41, 42, 43, 46, 47, 50, 60):
        assert (by_len[L] & F.FR_DGRAM != 0).any(), L
    for L in (42, 43, 46, 47, 50, 60):
        assert (by_len[L] & F.FR_ARP != 0).any() and (by_len[L] & F.FR_ARP_OK != 0).any(), L
    assert all((by_len[L] & F.FR_ARP_OK == 0).all() for L in (14, 15, 29, 30, 33, 34, 35, 41))


def test_dgram_lattice_classes():
    dgrams, res, shape = LH.dgram_targets()
    assert sorted({len(d) for d in dgrams}) == LH.DGRAM_LENGTHS
    assert {(len(d), int(r)) for d, r in zip(dgrams, res)} == {(L, r) for L in LH.DGRAM_LENGTHS for r in range(16)}
    # every length class meets every (hlen, data offset) pair; the options path meets every TCP start residue mod 4
    assert {(len(d), s) for d, s in zip(dgrams, shape)} == {(L, p) for L in LH.DGRAM_LENGTHS for p in LH.PAIRS}
    for h in (6, 15):
        assert {(int(r) + 4 * h) % 4 for r, s in zip(res, shape) if s[0] == h} == {0, 1, 2, 3}
        assert {int(r) for r, s in zip(res, shape) if s[0] == h} == set(range(16))
    # the shape bytes are what the generator was asked for, wherever the bytes exist and no bit was flipped since
    asked = sum(1 for d, (h, _) in zip(dgrams, shape) if len(d) >= 20 and d[0] & 15 == h)
    assert asked > 0.85 * sum(1 for d in dgrams if len(d) >= 20)
    nb = LH.n_batches(len(dgrams))
    assert nb == 75
    last, held = set(), set()
    for b in range(nb):
        items, off, which = LH.batch(dgrams, res, b, seed=2)
        at = _starts(off, which)
        assert sorted(at) == list(range(len(dgrams)))
        for t, (s, ln) in at.items():
            assert s % 16 == res[t] and ln == len(dgrams[t])
            held.add(LH.blocks_held(s, ln))
        assert all(len(x) < 16 for x, t in zip(items, which) if t < 0)
        assert which[-1] == 3 * b and int(off[-1]) == sum(len(x) for x in items)
        last.add(int(which[-1]))
    assert len(last) == nb and 3 * len(last) >= len(dgrams)
    assert held == {2, 3, 4, 5, 6}
    assert {len(dgrams[t]) for t in last} == set(LH.DGRAM_LENGTHS)
    assert {shape[t][0] for t in last} == set(LH.HLENS) and {shape[t][1] for t in last} == set(LH.DOFFS)


def test_dgram_lattice_status_classes():
    dgrams, _, shape = LH.dgram_targets()
    rec = P.unwrap_expect(dgrams)
    P.assert_unwrap_classes(rec, dgrams)
    st = rec[:, 36]
    parsed = (st & 7) == 7
    # a parsed record on every header length, and with the payload clamped to the datagram (doff 15 in 80 bytes)
    for h in LH.HLENS:
        assert any(p and s[0] == h and d[0] & 15 == h for p, s, d in zip(parsed, shape, dgrams)), h
    po = rec[:, 28:32].copy().view("<u4")[:, 0]
    pl = rec[:, 32:36].copy().view("<u4")[:, 0]
    lens = np.array([len(d) for d in dgrams])
    assert (po[parsed] + pl[parsed] == lens[parsed]).all()
    assert (parsed & (pl == 0)).any() and (parsed & (pl > 0)).any()


def test_periodic_inputs():
    """periodic.py's K items: K prime, every status class of every family present, lengths within the layout"""
    import test_gpu_frames as F

    assert all(P.K % k for k in range(2, 65)) and P.K > 4096
    router, rneigh = _hop_refs()
    frames, ins = P.frame_items()
    assert len(frames) == P.K and {len(f) for f in frames} == {P.FRAME_LEN} and P.FRAME_LEN <= P.FRAME_STRIDE
    P.assert_frame_classes(F.expect(frames, ins, router, rneigh)[0])
    dgrams = P.dgram_items()
    st, _, _, hd, after = P.route_expect(dgrams, router)
    P.assert_route_classes(st)
    assert [len(a) for a in after] == [len(d) for d in dgrams]
    assert all(a[:20] == bytes(h) for a, h, s in zip(after, hd, st) if s)
    udg = P.unwrap_items()
    P.assert_unwrap_classes(P.unwrap_expect(udg), udg)
    addrs = P.addr_items(F.ROUTES)
    m, f, _ = router.answers(addrs)
    assert addrs.size == P.K and 0 < m.sum() < P.K and {0, 1, 2, 3, 9} <= set(f.tolist())
    # the grid-stride batch sizes: a second trip of 256 full blocks and one partial wave
    for n, per_block in (((1 << 24) + 65573, 256), ((1 << 23) + 32805, 128)):
        rest = n - 65536 * per_block
        assert rest // per_block == 256 and rest % per_block == 37
    assert P.SWEEP_NS[:131] == list(range(131)) and {255, 256, 257, 511, 512, 513} <= set(P.SWEEP_NS)
