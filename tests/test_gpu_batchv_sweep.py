"""GPU: the arithmetic of the multi-batch launches (ics_checksum_batchv /
ics_ipv4_tcp_batchv) on its edges, against the oracle, bit-exact.

tests/batchv_plan.py generates the calls and models the grouping;
tests/test_batchv_plan.py proves from the inputs what they cover.  Here they
run, on the release library and on libicsum_debug.so (the block budget: release
only):

  block edges   per (entry, class) seven calls of 16 batches whose sizes put 1,
                per - 1, per, per + 1, 2 per - 1, 2 per and 2 per + 1 segments
                (per = the class's segments per block) into the first, the last
                and an inner slot of the launch's table; every batch has its own
                bytes and its own length inside the class;
  group cuts    1, 2, 15, 16, 17, 31, 32 and 33 batches of one class, and one
                call of about 100 descriptors, the classes in turn with empty
                batches (n = 0, null pointers) first, last and in between; a
                sample also against single calls on the same arguments;
  class edges   one batch on either side of each threshold, the class reported;
  null outputs  ics_ipv4_tcp_batchv with every subset of its outputs absent;
  the bodies    each class body as block lb of nb (not of a grid of its own):
                stride-1 batches of 144 starts, 16 lengths per call around the
                body's pass boundaries;
  the budget    five line64 batches of 4 x 4 194 303 segments (four fill a launch
                to 2^24 - 4 blocks, the fifth is cut off by the block budget), one
                of a segment more (runs alone), and two such datagram batches.

All outputs of a call are carved from one sentinel-filled allocation per output
kind with 8 guard elements around each, and the whole allocation is compared.
ics_dispatch_info must report "batchv", the class of the call's last launch as
the model plans it, and the call's batch count."""
import ctypes

import numpy as np
import pytest

import batchv_plan as bp
import lattice
import periodic
from conftest import engine_with
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

GUARD = 8
SENT = {"int16": 0x5A5A, "uint8": 0x5A}


@pytest.fixture(scope="module", params=[False, True], ids=["release", "debug"])
def eng(request):
    yield from engine_with(None, debug=request.param)


class _Carved:
    """k outputs of ns[j] elements in one sentinel-filled allocation, GUARD
    sentinels before, between and behind them"""

    def __init__(self, ns, dtype):
        import torch

        self.ns, self.pos, at = list(ns), [], GUARD
        for n in self.ns:
            self.pos.append(at)
            at += n + GUARD
        self.name = str(dtype).split(".")[-1]
        self.whole = torch.full((at,), SENT[self.name], dtype=dtype, device="cuda:0")

    def view(self, j):
        return self.whole[self.pos[j]:self.pos[j] + self.ns[j]]

    def check(self, tag, wants):
        """the whole allocation: wants[j] (None: not written) in place j, sentinels everywhere else"""
        udt = np.uint16 if self.name == "int16" else np.uint8
        want = np.full(self.whole.numel(), SENT[self.name], dtype=udt)
        for j, w in enumerate(wants):
            if w is not None:
                want[self.pos[j]:self.pos[j] + self.ns[j]] = w
        got = self.whole.cpu().numpy().view(udt)
        if not (got == want).all():
            i = int(np.flatnonzero(got != want)[0])
            j = max([x for x in range(len(self.pos)) if self.pos[x] - GUARD <= i], default=0)
            raise AssertionError(f"{tag}: batch {j} (n = {self.ns[j]}), element {i - self.pos[j]}: "
                                 f"{int(got[i]):#x}, want {int(want[i]):#x}")


def _upload(spec):
    """(the whole device buffer, the batch's view of it): the view's address mod 16 is the model's base"""
    if spec["n"] == 0:
        return None, None
    whole = _t(spec["buf"])
    view = whole[spec["lead"]:]
    assert view.data_ptr() % 16 == spec["lead"] % 16
    return whole, view


def _report(eng, entry, call, tag):
    _, alone, last = bp.plan([bp.desc(s) for s in call], entry)
    assert not alone and last is not None
    info = eng.dispatch_info()
    assert (info["kernel"], info["lps"], info["unroll"]) == ("batchv", last, len(call)), (tag, info)


def _opt(a):
    return None if a is None else _t(a)


def _run_checksum(eng, orc, call, tag, single_every=0):
    import torch

    devs = [_upload(s)[1] for s in call]
    outs = _Carved([s["n"] for s in call], torch.int16)
    batches = [dict(data=d, n=s["n"], stride=s["stride"], seg_len=s["seg_len"], offsets=_opt(s["offsets"]),
                    init=_opt(s["init"]), out=outs.view(j) if s["n"] else None)
               for j, (d, s) in enumerate(zip(devs, call))]
    eng.checksum_batchv(batches)
    torch.cuda.synchronize()
    _report(eng, "checksum", call, tag)
    wants = [bp.expect(orc, "checksum", s) if s["n"] else None for s in call]
    outs.check(tag, wants)
    if single_every:  # the header's contract: what k single calls on the same arguments give
        for j in range(1, len(call), single_every):
            b = batches[j]
            if b["n"]:
                one = eng.checksum_batch(b["data"], n=b["n"], offsets=b["offsets"], stride=b["stride"],
                                         seg_len=b["seg_len"], init=b["init"])
                assert (one.cpu().numpy().view(np.uint16) == wants[j]).all(), (tag, "single call", j)


def _run_ipv4(eng, orc, call, tag, modes=(0, 1, 2), single_every=0):
    import torch

    ups = [_upload(s) for s in call]
    ns = [s["n"] for s in call]
    for mode in modes:  # PATCH last: the read-only modes see the bytes as uploaded
        ip, tcp, st = _Carved(ns, torch.int16), _Carved(ns, torch.int16), _Carved(ns, torch.uint8)
        batches = [dict(dgrams=v, n=s["n"], stride=s["stride"], dgram_len=s["seg_len"], offsets=_opt(s["offsets"]),
                        ip_ck=ip.view(j) if s["n"] else None, tcp_ck=tcp.view(j) if s["n"] else None,
                        status=st.view(j) if s["n"] else None) for j, ((_, v), s) in enumerate(zip(ups, call))]
        eng.ipv4_tcp_batchv(batches, mode)
        torch.cuda.synchronize()
        _report(eng, "ipv4", call, (tag, mode))
        wants = [bp.expect(orc, "ipv4", s, mode) if s["n"] else None for s in call]
        for k, carved, what in ((0, ip, "ip_ck"), (1, tcp, "tcp_ck"), (2, st, "status")):
            carved.check(f"{tag} mode {mode} {what}", [None if w is None else w[k] for w in wants])
        for j, ((whole, _), w) in enumerate(zip(ups, wants)):
            if w is not None:  # COMPUTE, VERIFY: unchanged; PATCH: the oracle's bytes
                assert (whole.cpu().numpy() == w[3]).all(), (tag, mode, j, "datagram bytes")
        if single_every and mode == 0:
            for j in range(1, len(call), single_every):
                b = batches[j]
                if b["n"]:
                    one = eng.ipv4_tcp_batch(b["dgrams"], 0, n=b["n"], offsets=b["offsets"], stride=b["stride"],
                                             dgram_len=b["dgram_len"])
                    for k in range(3):
                        assert (one[k].cpu().numpy().view(wants[j][k].dtype) == wants[j][k]).all(), (tag, "single", j)


_RUN = {"checksum": _run_checksum, "ipv4": _run_ipv4}


# ---------------------------------------------------------- block edges ----
@pytest.mark.parametrize("pair", bp.PAIRS, ids=bp.pair_id)
def test_block_edges_in_every_slot(eng, orc, pair):
    entry, cls = pair
    for r, call in enumerate(bp.edge_calls(orc, entry, cls)):
        _RUN[entry](eng, orc, call, f"{bp.pair_id(pair)} call {r}")


# ------------------------------------------------------------ group cuts ---
@pytest.mark.parametrize("k", bp.CUT_KS)
def test_group_cuts(eng, orc, k):
    for entry, cls in bp.PAIRS:
        tag = f"{bp.pair_id((entry, cls))} k {k}"
        if entry == "checksum":
            _run_checksum(eng, orc, bp.cut_call(orc, entry, cls, k), tag, single_every=5)
        else:
            _run_ipv4(eng, orc, bp.cut_call(orc, entry, cls, k), tag, modes=(0, 2), single_every=5)


@pytest.mark.parametrize("entry", ["checksum", "ipv4"])
def test_all_classes_interleaved_with_empties(eng, orc, entry):
    _RUN[entry](eng, orc, bp.mixed_call(orc, entry), f"mixed {entry}", single_every=7)


# ----------------------------------------------------------- class edges ---
def test_class_edges(eng, orc):
    for tag, entry, spec, cls in bp.class_edge_cases(orc):
        _RUN[entry](eng, orc, [spec], tag)
        assert eng.dispatch_info()["lps"] == cls, tag


# ---------------------------------------------------------- null outputs ---
DROPS = [(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]  # outputs absent: 0 ip_ck, 1 tcp_ck, 2 status


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["compute", "verify", "patch"])
def test_ipv4_null_outputs(eng, orc, mode):
    """16 batches (a one-lane and a 16-lane class batch per pattern), every
    subset of the three outputs absent — all three in PATCH only, where the
    call still writes the datagrams; what is present and the bytes are the
    oracle's, and the places of the absent outputs keep their sentinels"""
    import torch

    from tcpip_network_protocol_stack_amd import _lib
    from tcpip_network_protocol_stack_amd.engine import _stream

    rng = np.random.default_rng(0x0DD + mode)
    call, drops = [], []
    for p, drop in enumerate(DROPS):
        for cls, n in ((bp.LANE1, 300 + p), (bp.LINE16, 40 + p)):
            call.append(bp.make_batch(orc, rng, "ipv4", cls, n, p))
            drops.append(drop if len(drop) < 3 or mode == 2 else ())
    ups = [_upload(s) for s in call]
    ns = [s["n"] for s in call]
    carved = [_Carved(ns, torch.int16), _Carved(ns, torch.int16), _Carved(ns, torch.uint8)]
    offs = [_opt(s["offsets"]) for s in call]
    arr = (_lib.DgramBatch * len(call))()
    for j, (s, (_, v)) in enumerate(zip(call, ups)):
        ptr = [None if k in drops[j] else carved[k].view(j).data_ptr() for k in range(3)]
        arr[j] = _lib.DgramBatch(v.data_ptr(), None if offs[j] is None else offs[j].data_ptr(), s["stride"],
                                 s["seg_len"], s["n"], ptr[0], ptr[1], ptr[2])
    eng._check(eng.lib.ics_ipv4_tcp_batchv(eng.ctx, arr, len(call), mode, _stream(None, eng.device)))
    torch.cuda.synchronize()
    _report(eng, "ipv4", call, mode)
    wants = [bp.expect(orc, "ipv4", s, mode) for s in call]
    for k, what in enumerate(("ip_ck", "tcp_ck", "status")):
        carved[k].check(f"mode {mode} {what}", [None if k in drops[j] else w[k] for j, w in enumerate(wants)])
    for j, ((whole, _), w) in enumerate(zip(ups, wants)):
        assert (whole.cpu().numpy() == w[3]).all(), (mode, j, "datagram bytes")
    if mode == 2:  # the batches without any output were patched
        assert all((wants[j][3] != call[j]["buf"]).any() for j in range(len(call)) if len(drops[j]) == 3)


# ------------------------------------------- the bodies behind a table -----
@pytest.fixture(scope="module")
def table_inputs():
    out = {}
    for nibble5 in (False, True):
        buf = bp.table_buffer(nibble5)
        out[nibble5] = (buf, _t(buf))
    rng = np.random.default_rng(0x7AB)
    init = rng.integers(0, 2**32, lattice.STARTS, dtype=np.uint64).astype(np.uint32)
    out["init"] = (init, _t(init))
    return out


@pytest.mark.parametrize("cls", [bp.TINY, bp.SMALL, bp.LINE16, bp.LINE64], ids=lambda c: bp.NAMES[c])
def test_checksum_bodies_behind_a_table(eng, orc, table_inputs, cls):
    """16 stride-1 batches of 144 consecutive starts per call, one length each
    (every other one with inits): each body runs as block lb of nb of its
    batch, at every start residue on either side of its pass boundaries"""
    import torch

    n = lattice.STARTS
    (buf, d), (init, dinit) = table_inputs[False], table_inputs["init"]
    for lengths in bp.table_lengths(cls):
        outs = _Carved([n] * len(lengths), torch.int16)
        eng.checksum_batchv([dict(data=d, n=n, stride=1, seg_len=L, init=dinit if j % 2 else None, out=outs.view(j))
                             for j, L in enumerate(lengths)])
        torch.cuda.synchronize()
        info = eng.dispatch_info()
        assert (info["kernel"], info["lps"], info["unroll"]) == ("batchv", cls, len(lengths)), (lengths, info)
        outs.check(f"{bp.NAMES[cls]} lengths {lengths[0]}..",
                   [orc.checksum_batch(buf, n, stride=1, seg_len=L, init=init if j % 2 else None)
                    for j, L in enumerate(lengths)])


@pytest.mark.parametrize("cls", [bp.LANE1, bp.LINE16, bp.LINE64], ids=lambda c: bp.NAMES[c])
def test_ipv4_bodies_behind_a_table(eng, orc, table_inputs, cls):
    """the same for the fused entry's read-only modes (about half of the bytes
    read as a header length of 5); the buffer stays as it was"""
    import torch

    n = lattice.STARTS
    buf, d = table_inputs[True]
    for lengths in bp.table_lengths(cls):
        for mode in (0, 1):
            carved = [_Carved([n] * len(lengths), torch.int16), _Carved([n] * len(lengths), torch.int16),
                      _Carved([n] * len(lengths), torch.uint8)]
            eng.ipv4_tcp_batchv([dict(dgrams=d, n=n, stride=1, dgram_len=L, ip_ck=carved[0].view(j),
                                      tcp_ck=carved[1].view(j), status=carved[2].view(j))
                                 for j, L in enumerate(lengths)], mode)
            torch.cuda.synchronize()
            info = eng.dispatch_info()
            assert (info["kernel"], info["lps"], info["unroll"]) == ("batchv", cls, len(lengths)), (lengths, info)
            host = buf.copy()
            wants = [orc.ipv4_tcp_batch(host, n, mode, stride=1, dgram_len=L) for L in lengths]
            assert (host == buf).all()
            for k, what in enumerate(("ip_ck", "tcp_ck", "status")):
                carved[k].check(f"{bp.NAMES[cls]} mode {mode} {what} lengths {lengths[0]}..", [w[k] for w in wants])
    assert (d.cpu().numpy() == buf).all()


# ------------------------------------------- block budget and "alone" ------
def _same(whole, n, want, sent, tag):
    """as test_gpu_grid_stride: the first n elements equal `want` on the device, the tail is untouched"""
    import torch

    got = whole[:n]
    if not torch.equal(got, want):
        i = int((got != want).nonzero()[0])
        raise AssertionError(f"{tag}: element {i} (of {n}) is {int(got[i]):#x}, want {int(want[i]):#x}")
    assert periodic.tail_untouched(whole, n, sent), f"{tag}: written behind the output"


def _budget_batches(orc, rng, count, n):
    """`count` batches of n segments of BUDGET_LEN bytes at stride 0 (every
    segment reads the batch's one copy of its bytes), each with its own bytes
    and a per-segment init array of period periodic.K (4099, a prime: the
    period lines up with no block); the expectation is the oracle's value for
    each init of the period, repeated on the device"""
    import torch

    out = []
    for _ in range(count):
        buf = rng.integers(0, 256, bp.BUDGET_LEN + 16, dtype=np.uint8)
        init = rng.integers(0, 2**32, periodic.K, dtype=np.uint64).astype(np.uint32)
        want = orc.checksum_batch(buf, periodic.K, stride=0, seg_len=bp.BUDGET_LEN, init=init)
        whole, view = periodic.sentinel(n, torch.int16, SENT["int16"])
        out.append(dict(data=_t(buf), n=n, stride=0, seg_len=bp.BUDGET_LEN, init=periodic.tile(_t(init), n), out=view,
                        whole=whole, want=periodic.tile(_t(want), n)))
    return out


def test_block_budget_cuts_a_launch(engine, orc):
    """five batches of 4 x 4 194 303 segments: four fill one launch to 2^24 - 4
    blocks, the fifth does not fit (kMaxBlocks = 2^24 - 1) and takes a launch of
    its own — block indices up to 2^24 - 5 through bv_find, and `blocks + nb >
    kMaxBlocks` on its edge"""
    import torch

    n = bp.budget_n()
    launches, alone, last = bp.plan([bp.budget_desc(n)] * 5, "checksum")
    assert [len(g) for _, g in launches] == [4, 1] and not alone
    batches = _budget_batches(orc, np.random.default_rng(0xB0D6E7), 5, n)
    assert len({bytes(b["want"][:8].cpu().numpy()) for b in batches}) == 5  # no two batches agree
    engine.checksum_batchv(batches)
    torch.cuda.synchronize()
    info = engine.dispatch_info()
    assert (info["kernel"], info["lps"], info["unroll"]) == ("batchv", last, 5), info
    for j, b in enumerate(batches):
        _same(b["whole"], n, b["want"], SENT["int16"], f"batch {j}")


def test_a_batch_past_a_quarter_of_the_budget_runs_alone(engine, orc):
    """one segment more than the largest batch that shares a launch: the single-batch path, beside a small batch"""
    import torch

    n = bp.budget_n() + 1
    assert bp.plan([bp.budget_desc(9), bp.budget_desc(n)], "checksum") == ([(bp.LINE64, [0])], [1], bp.LINE64)
    rng = np.random.default_rng(0xA10E)
    small = _budget_batches(orc, rng, 1, 9)
    big = _budget_batches(orc, rng, 1, n)
    engine.checksum_batchv(big)  # alone and nothing else: the report is the single call's
    torch.cuda.synchronize()
    assert engine.dispatch_info()["kernel"] == "checksum"
    _same(big[0]["whole"], n, big[0]["want"], SENT["int16"], "alone")
    big[0]["whole"].fill_(SENT["int16"])
    engine.checksum_batchv(small + big)
    torch.cuda.synchronize()
    info = engine.dispatch_info()
    assert (info["kernel"], info["lps"], info["unroll"]) == ("batchv", bp.LINE64, 2), info
    _same(small[0]["whole"], 9, small[0]["want"], SENT["int16"], "the small batch")
    _same(big[0]["whole"], n, big[0]["want"], SENT["int16"], "alone, beside a launch")


def test_block_budget_ipv4_verify(engine, orc):
    """two datagram batches of 4 x 4 194 303 in one VERIFY launch (2^23 - 2
    blocks, the second batch's blocks found past 2^22): one datagram each at
    stride 0, one that verifies and one that does not"""
    import torch

    n = bp.budget_n()
    assert bp.plan([bp.budget_desc(n)] * 2, "ipv4") == ([(bp.LINE64, [0, 1])], [], bp.LINE64)
    rng = np.random.default_rng(0x4E71F)
    rows = bp.fixed_datagrams(orc, rng, 1, bp.BUDGET_LEN)  # row 0 carries the oracle's checksums
    bad = rows.copy()
    bad[0, bp.BUDGET_LEN - 1] ^= 0x40
    batches, wants = [], []
    for row in (rows[0], bad[0]):
        buf = np.concatenate([row, np.zeros(16, np.uint8)])
        wants.append([w[0] for w in orc.ipv4_tcp_batch(buf, 1, 1, stride=0, dgram_len=bp.BUDGET_LEN)])
        outs = [periodic.sentinel(n, dt, SENT[nm]) for dt, nm in ((torch.int16, "int16"), (torch.int16, "int16"),
                                                                 (torch.uint8, "uint8"))]
        batches.append(dict(dgrams=_t(buf), n=n, stride=0, dgram_len=bp.BUDGET_LEN, ip_ck=outs[0][1], tcp_ck=outs[1][1],
                            status=outs[2][1], wholes=[o[0] for o in outs]))
    assert wants[0][2] == 0x0F and wants[1][2] != 0x0F
    engine.ipv4_tcp_batchv(batches, 1)
    torch.cuda.synchronize()
    info = engine.dispatch_info()
    assert (info["kernel"], info["lps"], info["unroll"]) == ("batchv", bp.LINE64, 2), info
    for j, (b, w) in enumerate(zip(batches, wants)):
        for k, (nm, dt) in enumerate((("int16", np.uint16), ("int16", np.uint16), ("uint8", np.uint8))):
            whole = b["wholes"][k]
            want = _t(np.array([w[k]], dtype=dt)).expand(n)
            _same(whole, n, want, SENT[nm], f"batch {j} output {k}")
