"""CPU: the calls of tests/test_gpu_batchv_sweep.py reach what that module
claims, proven from the inputs alone with the model of tests/batchv_plan.py
(no kernel): the block edges of every (entry, class) at the first, the last
and an inner slot of a full launch, the group cuts, the class edges, the
block budget, and batches that a block serving the wrong batch cannot get
right.  The model's constants are the sources' (read as text).  If a
generator is thinned below one of these conditions, or a constant of
icsum_batchv.h / run_batchv / pick_geometry changes, a test here fails."""
import numpy as np
import pytest

import batchv_plan as bp
import lattice

C = bp.C


def _all_calls(orc):
    """(tag, entry, specs) of every generated call"""
    for entry, cls in bp.PAIRS:
        for r, call in enumerate(bp.edge_calls(orc, entry, cls)):
            yield f"edge-{bp.pair_id((entry, cls))}-{r}", entry, call
        for k in bp.CUT_KS:
            yield f"cut-{bp.pair_id((entry, cls))}-{k}", entry, bp.cut_call(orc, entry, cls, k)
    for entry in ("checksum", "ipv4"):
        yield f"mixed-{entry}", entry, bp.mixed_call(orc, entry)


# ------------------------------------------------------------ constants ----
def test_the_models_constants_are_the_sources():
    assert C["classes"] == {"kBvDense64": 0, "kBvTiny": 1, "kBvSmall": 2, "kBvLine16": 3, "kBvLine64": 4, "kBvLane1": 5}
    assert C["max_batchv"] == 16
    assert C["per"] == {bp.DENSE: 256, bp.TINY: 256, bp.LANE1: 256, bp.SMALL: 128, bp.LINE16: 16, bp.LINE64: 4}
    assert C["max_blocks"] == 2**24 - 1 and C["alone_div"] == 4 and C["table_limit"] == 2**24
    assert C["max_blocks"] < C["table_limit"]  # what run_batchv may pass, bv_table accepts
    assert C["tiny_max"] == 56 and C["tiny_geometry"] == (1, 4, 4, 1)
    assert C["offsets_hint"] == 65536 and C["dense_len"] == 64 and C["dense_lens"] == [32, 64, 128]
    assert C["line64_from"] == 32
    # pick_geometry's chunk thresholds, and where the classes change along them
    assert [s[0] for s in C["steps"]] == [5, 9, 17, 56, 69, 82, 120, 140, 220, None]
    assert [s[4] > 1 for s in C["steps"]] == [True] * 3 + [False] * 7
    assert [s[1] for s in C["steps"]] == [4, 4, 8, 16, 16, 16, 16, 16, 32, 64]


def test_per_block_is_what_each_body_covers():
    """256 threads: one lane per segment (tiny, lane1); 64 four-lane groups x 4
    segments in flight (dense); 64 groups x 2 (small); 256 / lanes (line grids)"""
    assert bp.per_block(bp.TINY) == bp.per_block(bp.LANE1) == 256
    assert bp.per_block(bp.DENSE) == (256 // 4) * 4
    assert bp.per_block(bp.SMALL) == (256 // 4) * 2
    assert bp.per_block(bp.LINE16) == 256 // 16 and bp.per_block(bp.LINE64) == 256 // 64
    for cls, (lps, _, _, _) in bp.BODY.items():
        assert bp.per_block(cls) == (256 // lps) * (2 if cls == bp.SMALL else 1)


def test_class_thresholds():
    d = lambda L, **kw: dict(dict(n=9, stride=L, seg_len=L, offsets=False, base=0), **kw)  # noqa: E731
    edges = {0: bp.TINY, 56: bp.TINY, 57: bp.SMALL, 272: bp.SMALL, 273: bp.LINE16, 2240: bp.LINE16, 2241: bp.LINE64,
             3520: bp.LINE64, 3521: bp.LINE64, 65535: bp.LINE64}
    for L, cls in edges.items():
        assert bp.cls_checksum(d(L, stride=L + 1)) == cls, L
        assert bp.cls_ipv4(d(L)) == {bp.TINY: bp.LANE1, bp.SMALL: bp.LINE16}.get(cls, cls), L
    assert bp.cls_checksum(d(64)) == bp.DENSE
    assert bp.cls_checksum(d(64, base=1)) == bp.cls_checksum(d(64, stride=72)) == bp.SMALL
    assert bp.cls_checksum(d(32)) == bp.TINY and bp.cls_checksum(d(128)) == bp.SMALL
    assert bp.cls_checksum(d(0, offsets=True)) == bp.LINE64 and bp.cls_ipv4(d(0, offsets=True)) == bp.LINE16


def test_class_edge_cases_are_of_the_named_classes(orc):
    cases = bp.class_edge_cases(orc)
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids) == 17
    for tag, entry, spec, cls in cases:
        assert bp.CLS_OF[entry](bp.desc(spec)) == cls, tag
        assert bp.blocks(cls, spec["n"]) >= 2 and spec["n"] % bp.per_block(cls), tag
        assert bp.plan([bp.desc(spec)], entry) == ([(cls, [0])], [], cls), tag
    assert {c[3] for c in cases if c[1] == "checksum"} == set(bp.ENTRY_CLASSES["checksum"])
    assert {c[3] for c in cases if c[1] == "ipv4"} == set(bp.ENTRY_CLASSES["ipv4"])


# ---------------------------------------------------------- block edges ----
@pytest.mark.parametrize("pair", bp.PAIRS, ids=bp.pair_id)
def test_block_edges_at_the_first_last_and_an_inner_slot(orc, pair):
    entry, cls = pair
    per = bp.per_block(cls)
    sizes = bp.edge_sizes(per)
    assert sizes == [1, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1] and len(set(sizes)) == 7
    seen = {0: set(), 15: set(), "inner": set()}
    lens, one_block_run, with_init, offsets_batches = set(), 0, set(), 0
    for call in bp.edge_calls(orc, entry, cls):
        descs = [bp.desc(s) for s in call]
        launches, alone, last = bp.plan(descs, entry)
        assert launches == [(cls, list(range(16)))] and not alone and last == cls  # one full launch of this class
        run = 0
        for slot, s in enumerate(call):
            seen[slot if slot in (0, 15) else "inner"].add(s["n"])
            run = run + 1 if bp.blocks(cls, s["n"]) == 1 else 0
            one_block_run = max(one_block_run, run)
            lens.add(s["seg_len"])
            with_init.add(s["init"] is not None)
            offsets_batches += s["offsets"] is not None
    for where, got in seen.items():
        assert got == set(sizes), (where, sorted(set(sizes) - got))
    assert one_block_run >= 3  # 1, per - 1 and per side by side: three blocks in a row, three batches
    assert lens - {0} == set(bp.LENGTHS[cls])
    assert with_init == ({False, True} if entry == "checksum" else {False})
    assert (offsets_batches > 0) == (pair in (("checksum", bp.LINE64), ("ipv4", bp.LINE16)))


def test_a_thinned_edge_sweep_would_be_noticed(orc):
    # six of the seven calls leave one size out of slot 0 and one out of slot 15
    calls = bp.edge_calls(orc, "checksum", bp.SMALL)[:6]
    assert len({c[0]["n"] for c in calls}) == 6 and len({c[15]["n"] for c in calls}) == 6


def test_block_table_and_search():
    """the model's bv_table / bv_find on the edge sizes: every block of the
    concatenated grid belongs to the batch whose [block0, block0 + nblk) holds it"""
    for cls in (bp.SMALL, bp.LINE64):
        per = bp.per_block(cls)
        ns = [bp.edge_sizes(per)[s % 7] for s in range(16)]
        block0, nblk = bp.block_table(cls, ns)
        assert block0[0] == 0 and all(b > a for a, b in zip(block0, block0[1:]))
        for n, nb in zip(ns, nblk):
            assert (nb - 1) * per < n <= nb * per
        owner = [j for j, nb in enumerate(nblk) for _ in range(nb)]
        assert [bp.find(block0, blk) for blk in range(sum(nblk))] == owner
        short = block0[:5] + [0xFFFFFFFF] * 11  # a launch of five: the padding is never at or below a block
        assert [bp.find(short, blk) for blk in range(sum(nblk[:5]))] == owner[:sum(nblk[:5])]


# ------------------------------------------------------------ group cuts ---
def test_every_plan_is_a_partition_within_both_caps(orc):
    ncalls = 0
    for tag, entry, call in _all_calls(orc):
        descs = [bp.desc(s) for s in call]
        launches, alone, last = bp.plan(descs, entry)
        want = [j for j, d in enumerate(descs) if d["n"]]
        got = sorted(alone + [j for _, g in launches for j in g])
        assert got == want, tag
        assert not alone, tag
        for cls, g in launches:
            assert 1 <= len(g) <= C["max_batchv"] and g == sorted(g), tag
            assert all(bp.CLS_OF[entry](descs[j]) == cls for j in g), tag
            assert sum(bp.blocks(cls, descs[j]["n"]) for j in g) <= C["max_blocks"], tag
        assert [c for c, _ in launches] == sorted(c for c, _ in launches), tag
        for (ca, ga), (cb, gb) in zip(launches, launches[1:]):  # a cut inside a class: only at a full launch
            assert ca != cb or len(ga) == C["max_batchv"], tag
        assert last == launches[-1][0], tag
        ncalls += 1
    assert ncalls == 8 * (7 + len(bp.CUT_KS)) + 2


@pytest.mark.parametrize("pair", bp.PAIRS, ids=bp.pair_id)
def test_group_cut_calls(orc, pair):
    entry, cls = pair
    assert bp.CUT_KS == (1, 2, 15, 16, 17, 31, 32, 33)
    for k in bp.CUT_KS:
        call = bp.cut_call(orc, entry, cls, k)
        launches, alone, last = bp.plan([bp.desc(s) for s in call], entry)
        full, rest = divmod(k, 16)
        assert [len(g) for _, g in launches] == [16] * full + [rest] * (rest > 0), k
        assert [j for _, g in launches for j in g] == list(range(k)) and {c for c, _ in launches} == {cls}


@pytest.mark.parametrize("entry", ["checksum", "ipv4"])
def test_mixed_call_interleaves_every_class_and_empties(orc, entry):
    call = bp.mixed_call(orc, entry)
    assert 100 <= len(call) <= 110
    empty = [j for j, s in enumerate(call) if s["n"] == 0]
    assert empty[0] == 0 and empty[-1] == len(call) - 1 and len(empty) >= 8
    assert all(call[j]["buf"] is None for j in empty)
    descs = [bp.desc(s) for s in call]
    cls = [bp.CLS_OF[entry](d) for d in descs if d["n"]]
    classes = bp.ENTRY_CLASSES[entry]
    assert cls == [classes[j % len(classes)] for j in range(len(cls))]  # round-robin
    launches, alone, last = bp.plan(descs, entry)
    assert not alone and last == max(classes)
    assert [c for c, _ in launches] == [c for c in sorted(classes) for _ in range(2)]  # a cut inside every class
    assert all(len(g) == 16 for _, g in launches[::2])
    for _, g in launches:  # batches of one launch are not neighbours in the call
        assert all(b - a >= len(classes) for a, b in zip(g, g[1:]))


def test_block_budget_and_alone():
    n = bp.budget_n()
    assert n == 4 * 4194303 and bp.cls_checksum(bp.budget_desc(n)) == bp.cls_ipv4(bp.budget_desc(n)) == bp.LINE64
    assert bp.blocks(bp.LINE64, n) == C["max_blocks"] // 4
    launches, alone, last = bp.plan([bp.budget_desc(n)] * 5, "checksum")
    assert launches == [(bp.LINE64, [0, 1, 2, 3]), (bp.LINE64, [4])] and not alone and last == bp.LINE64
    assert 4 * bp.blocks(bp.LINE64, n) == 2**24 - 4  # the fifth batch does not fit: the block budget cuts
    assert 4 < C["max_batchv"]  # ... not the batch count
    assert bp.plan([bp.budget_desc(n + 1)], "checksum") == ([], [0], None)
    assert bp.plan([bp.budget_desc(9), bp.budget_desc(n + 1)], "checksum") == ([(bp.LINE64, [0])], [1], bp.LINE64)
    assert bp.plan([bp.budget_desc(n)] * 2, "ipv4") == ([(bp.LINE64, [0, 1])], [], bp.LINE64)


# ------------------------------------ a block that serves the wrong batch ---
def _outputs(orc, entry, spec):
    w = bp.expect(orc, entry, spec)
    return w if entry == "checksum" else np.stack([w[0], w[1], w[2].astype(np.uint16)], axis=1)


def test_no_two_batches_of_a_launch_agree(orc):
    """a block that ran with a neighbour's descriptor (or any other batch's
    of its launch) writes values that differ from the expected ones: over
    their common prefix no two batches of one launch have the same outputs,
    and no two share their bytes"""
    pairs = 0
    for tag, entry, call in _all_calls(orc):
        outs = {}
        for _, g in bp.plan([bp.desc(s) for s in call], entry)[0]:
            for j in g:
                outs[j] = _outputs(orc, entry, call[j])
            for x, a in enumerate(g):
                for b in g[x + 1:]:
                    m = min(call[a]["n"], call[b]["n"])
                    assert (outs[a][:m] != outs[b][:m]).any(), (tag, a, b)
                    assert call[a]["buf"] is not call[b]["buf"]
                    pairs += 1
    assert pairs > 10000


# ------------------------------------------------ the launch, emulated -----
def _sim_wants(ns):
    """a value per (batch, segment) that is never the sentinel"""
    w = [(j << 11) + np.arange(n, dtype=np.int64) + 1 for j, n in enumerate(ns)]
    assert all((x != bp.SIM_SENTINEL).all() for x in w)
    return w


def _sim_differs(cls, ns, mutation):
    wants = _sim_wants(ns)
    outs = bp.simulate(cls, ns, wants, mutation)
    return [j for j, (o, w) in enumerate(zip(outs, wants)) if (o != w).any()]


@pytest.mark.parametrize("pair", bp.PAIRS, ids=bp.pair_id)
def test_an_off_by_one_in_the_block_map_changes_the_compared_outputs(orc, pair):
    """bp.simulate runs a launch block by block.  Unmutated it writes every
    expected value of every generated launch; with `>` for `>=` in the search
    or the block's index one off, every block-edge call has batches whose
    outputs keep a sentinel (the whole allocation is compared, so any does);
    zero padding behind the last batch shows in every launch of fewer than 16
    batches; a block count rounded down shows for the dense body (no loop)
    and — since the other bodies stride by nb blocks — nowhere else."""
    entry, cls = pair
    for call in bp.edge_calls(orc, entry, cls):
        ns = [s["n"] for s in call]
        assert _sim_differs(cls, ns, None) == []
        assert _sim_differs(cls, ns, "pad_zero") == []  # a full launch has no padding
        for m in ("search_gt", "lb_plus_1", "lb_minus_1"):
            bad = _sim_differs(cls, ns, m)
            assert bad, m
            # the first (search, lb + 1) or the last (lb - 1) block of a batch is lost: slots 0 / 15 included
            if m == "lb_plus_1":
                assert bad == list(range(16))
            if m == "lb_minus_1":
                assert bad == list(range(16))
            if m == "search_gt":
                assert bad == list(range(1, 16))
        short = _sim_differs(cls, ns, "blocks_short")
        if cls == bp.DENSE:
            per = bp.per_block(cls)
            assert short == [j for j, n in enumerate(ns) if n > per and n % per]
            assert short
        else:
            assert short == []
    for k in bp.CUT_KS:
        ns = [s["n"] for s in bp.cut_call(orc, entry, cls, k)]
        for lo in range(0, k, 16):
            group = ns[lo:lo + 16]
            assert _sim_differs(cls, group, None) == []
            assert bool(_sim_differs(cls, group, "pad_zero")) == (len(group) < 16), (k, lo)


# ------------------------------------------- the bodies behind a table -----
@pytest.mark.parametrize("cls", [bp.SMALL, bp.LINE16, bp.LINE64], ids=lambda c: bp.NAMES[c])
def test_table_lengths_meet_every_pass_boundary(cls):
    """stride-1 batches of lattice.STARTS segments: the chunks a lane group
    walks land on k P - 1, k P and k P + 1 for each pass boundary swept, and
    every length stays inside the class"""
    lps, unroll, anchor, ks = bp.BODY[cls]
    calls = bp.table_lengths(cls)
    assert all(len(c) == 16 for c in calls) and len(calls) == 2 * len(ks)
    lengths = [L for c in calls for L in c]
    d = lambda L: dict(n=lattice.STARTS, stride=1, seg_len=L, offsets=False, base=0)  # noqa: E731
    assert {bp.cls_checksum(d(L)) for L in lengths} == {cls}
    if cls != bp.SMALL:
        assert {bp.cls_ipv4(d(L)) for L in lengths} == {cls}
    hit = lattice.stride1_classes(lps * unroll, anchor, lengths, ks=ks)
    assert hit.any(axis=(2, 3, 4)).all(), hit.any(axis=(2, 3, 4))
    assert {16 * k * lps * unroll for k in ks} <= set(lengths)


def test_table_lengths_of_the_one_lane_classes():
    calls = bp.table_lengths(bp.TINY)
    assert calls == bp.table_lengths(bp.LANE1) and all(len(c) == 16 for c in calls)
    assert {L for c in calls for L in c} == set(range(57))
    d = lambda L: dict(n=lattice.STARTS, stride=1, seg_len=L, offsets=False, base=0)  # noqa: E731
    assert {bp.cls_checksum(d(L)) for L in range(57)} == {bp.TINY} and {bp.cls_ipv4(d(L)) for L in range(57)} == {bp.LANE1}
    assert bp.table_buffer(False).size >= lattice.STARTS + bp.TABLE_LMAX and bp.TABLE_LMAX == 16384 + 7
