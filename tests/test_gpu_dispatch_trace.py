"""GPU: the device dispatch's decisions, pinned against a recorded trace.

csrc/icsum_dispatch.cpp picks the kernel and geometry of every device batch
from the batch's shape, the ICSUM_FORCE hooks and the plan cache.  The parity
suites check what the launches compute; this module checks *which* launch ran.
A case is (entry point, length mix, n, ICSUM_FORCE string): a fresh Engine
(an empty plan cache), three calls on the same device buffers with a stream
synchronise after each (so the plan word has landed and the next lookup is
deterministic), and after each call ics_dispatch_info's (kernel, lps, unroll,
plan) with the deltas of plan_hits / plan_misses / plan_requests.  The three
calls' outputs must be bit-identical (the miss and the hit path agree; parity
with the oracle is the other suites' job).  Two longer cases pin kPlanRefresh
(130 calls) and the LRU eviction over kPlanSlots (five offsets buffers).

tests/golden/dispatch_trace.json holds every case's trace, recorded on the
commit named inside it with

    python tests/test_gpu_dispatch_trace.py --record

and never re-recorded for a change that is meant to keep the dispatch as it
is.  A case missing from the fixture fails."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLD, ROOT, engine_with

FIXTURE = os.path.join(GOLD, "dispatch_trace.json")
SEED = 0x4D4958

ENTRIES = ["checksum_batch", "sum_batch_odd", "ipv4_tcp_batch", "tcp_wrap_batch", "tcp_wrap_headers"]
WRAPS = ("tcp_wrap_batch", "tcp_wrap_headers")
# offsets batches: ("ack", k) = 40-byte ACKs in k of every 16 segments, 1500 bytes the rest
OFFSET_MIXES = ["all40", "64to144", "ack3", "ack4", "ack8", "ack13", "uniform", "all1500", "mixed"]
# fixed-stride batches (stride == length); fixed64 is the dense kernel's shape
FIXED = {"fixed40": 40, "fixed1500": 1500, "fixed64": 64}
MIXES = OFFSET_MIXES + list(FIXED)
# both sides of every threshold of ics_ctx: kSmallPlanMin, bin_min / kTileMin,
# kTileMinChecksum, and (the wraps) kWrapTwoPassMin
NS = [16383, 16384, 65535, 65536, 131071, 131072]
NS_WRAP = NS + [262143, 262144]
N_BIG = 1048577  # past 2^20: the binned path's 32-lane last-bin rule
HOOKS = ["twoclass=16", "tile=1", "tile=0", "tile=1,twoclass=16", "bin=0", "bin=1", "bin_plan=0", "bin_plan=1",
         "bin_plan=2", "bin_plan=3", "last_bin_lps=32", "lps=16,unroll=8,mode=3", "wrap_passes=1", "wrap_passes=2",
         "span_segs=8"]
HOOK_MIXES = ["uniform", "ack8"]
HOOK_N = 65536
# the multi-batch calls' large batch: more than 2^22 - 1 blocks of its class
# (run_batchv's `alone` path: the full single-batch dispatch, plan cache included)
BV_ALONE = {"checksum_batchv": 4 << 22, "ipv4_tcp_batchv": 16 << 22}
REFRESH_CALLS, REFRESH_N = 130, 16384
EVICT_SEQ = [0, 1, 2, 3, 0, 1, 2, 3, 4, 1, 2, 3, 0, 4, 0]
EVICT_N = 16384


def key_of(entry, mix, n, force=""):
    return f"{entry}|{mix}|{n}|{force}"


def group_keys():
    """{group id: [case key, ...]} — one group per test case below"""
    groups = {}
    for e in ENTRIES:
        for m in MIXES:
            groups[f"sweep-{e}-{m}"] = [key_of(e, m, n) for n in (NS_WRAP if e in WRAPS else NS)]
        groups[f"big-{e}"] = [key_of(e, "all40", N_BIG)]
        for h in HOOKS:
            groups[f"hook-{e}-{h}"] = [key_of(e, m, HOOK_N, h) for m in HOOK_MIXES]
    for e, n in BV_ALONE.items():
        groups[f"batchv-{e}"] = [key_of(e, "3small+all40", n)]
    groups["refresh"] = [key_of("checksum_batch", "uniform", REFRESH_N, f"calls={REFRESH_CALLS}")]
    groups["evict"] = [key_of("checksum_batch", "uniform", EVICT_N, "buffers=5")]
    return groups


# ---- inputs ---------------------------------------------------------------
def _hash(i):
    """splitmix64 of the indices (numpy's own generators are not pinned across versions)"""
    with np.errstate(over="ignore"):
        z = (i.astype(np.uint64) + np.uint64(SEED)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mix_offsets(mix, n):
    """packed uint64 offsets (n + 1) of an offsets mix"""
    if mix == "mixed":  # icsw_mixed_len: 64 B .. 64 KiB
        from tcpip_network_protocol_stack_amd.engine import mixed_offsets

        return mixed_offsets(n, SEED)
    i = np.arange(n, dtype=np.uint64)
    if mix == "all40":
        lens = np.full(n, 40, dtype=np.uint64)
    elif mix == "all1500":
        lens = np.full(n, 1500, dtype=np.uint64)
    elif mix == "64to144":
        lens = np.uint64(64) + _hash(i) % np.uint64(81)
    elif mix == "uniform":
        lens = np.uint64(40) + _hash(i) % np.uint64(1001)
    else:  # ackK: exactly K of every 16 consecutive segments are ACKs
        k = int(mix[3:])
        lens = np.where((i * np.uint64(7)) % np.uint64(16) < np.uint64(k), 40, 1500).astype(np.uint64)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return off


class Inputs:
    """Device buffers shared by every case (the dispatch never looks at the
    bytes): one byte stream from the workload generator, message records, and
    each mix's offsets at its largest n (a case takes the first n + 1)."""

    def __init__(self):
        import torch

        from tcpip_network_protocol_stack_amd.engine import Engine

        self.torch = torch
        self.helper = Engine(0)  # fills and restores the bytes; never traced
        self.nbytes = max(int(mix_offsets("mixed", NS_WRAP[-1])[-1]), 40 * max(BV_ALONE.values()), 1500 * NS_WRAP[-1])
        self.bytes = self.helper.fill_bytes(torch.empty(self.nbytes + 64, dtype=torch.uint8, device="cuda:0"), SEED)
        self.msgs = self.helper.fill_bytes(torch.empty(28 * N_BIG, dtype=torch.uint8, device="cuda:0"), SEED + 1)
        self.odd = (torch.arange(N_BIG, device="cuda:0") & 1).to(torch.uint8)
        self._off = {}
        torch.cuda.synchronize()

    def offsets(self, mix, n):
        if mix not in self._off:
            top = N_BIG if mix == "all40" else NS_WRAP[-1]
            self._off[mix] = self.torch.from_numpy(mix_offsets(mix, top).view(np.int64)).cuda()
        return self._off[mix][: n + 1]

    def restore(self, nbytes):
        """the in-place wrap wrote headers into the stream: regenerate it"""
        self.helper.fill_bytes(self.bytes[:nbytes], SEED)
        self.torch.cuda.synchronize()

    def close(self):
        self.torch.cuda.synchronize()
        self.helper.close()


_inputs = None


def inputs():
    global _inputs
    if _inputs is None:
        _inputs = Inputs()
    return _inputs


# ---- one case ---------------------------------------------------------------
def _force_dict(force):
    return dict(kv.split("=") for kv in force.split(",")) if force else {}


def _call(eng, inp, entry, n, off, length):
    """one call of `entry`; returns the tensors that hold its results"""
    torch = inp.torch
    kw = dict(n=n, offsets=off) if off is not None else dict(n=n, stride=length)
    if entry == "checksum_batch":
        return [eng.checksum_batch(inp.bytes, seg_len=length, **kw)]
    if entry == "sum_batch_odd":
        return [eng.sum_batch(inp.bytes, seg_len=length, odd=inp.odd[:n], **kw)]
    if entry == "ipv4_tcp_batch":
        return list(eng.ipv4_tcp_batch(inp.bytes, 1, dgram_len=length, **kw))  # VERIFY: read-only
    msgs = inp.msgs[: 28 * n]
    ip = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    tcp = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    if entry == "tcp_wrap_headers":
        hdrs = torch.zeros(40 * n, dtype=torch.uint8, device="cuda:0")
        eng.tcp_wrap_headers(inp.bytes, msgs, hdrs, payload_len=length, ip_ck=ip, tcp_ck=tcp, **kw)
        return [hdrs, ip, tcp]
    assert entry == "tcp_wrap_batch", entry
    used = int(off[n]) if off is not None else n * length
    eng.tcp_wrap_batch(inp.bytes, msgs, dgram_len=length, ip_ck=ip, tcp_ck=tcp, **kw)
    torch.cuda.synchronize()
    out = [inp.bytes[:used].clone(), ip, tcp]
    inp.restore(used)
    return out


def _traced(eng, torch, calls):
    """run each thunk, synchronise, and record the launch and the counters' deltas"""
    rows, outs = [], []
    before = eng.dispatch_info()
    for call in calls:
        outs.append(call())
        torch.cuda.synchronize()
        d = eng.dispatch_info()
        rows.append([d["kernel"], d["lps"], d["unroll"], d["plan"], d["plan_hits"] - before["plan_hits"],
                     d["plan_misses"] - before["plan_misses"], d["plan_requests"] - before["plan_requests"]])
        before = d
    return rows, outs


def _same(outs, what):
    for k, o in enumerate(outs[1:], 1):
        for a, b in zip(outs[0], o):
            assert bool((a == b).all()), f"{what}: call {k + 1} differs from call 1"


def trace_single(entry, mix, n, force=""):
    inp = inputs()
    off = None if mix in FIXED else inp.offsets(mix, n)
    length = FIXED.get(mix, 0)
    for eng in engine_with(_force_dict(force)):
        rows, outs = _traced(eng, inp.torch, [lambda: _call(eng, inp, entry, n, off, length)] * 3)
        _same(outs, key_of(entry, mix, n, force))
    return rows


def trace_batchv(entry, n_alone):
    """three small fixed-length batches of different kernel shapes and one
    offsets batch (all 40 bytes) large enough to run alone"""
    inp = inputs()
    torch = inp.torch
    off = torch.arange(n_alone + 1, dtype=torch.int64, device="cuda:0") * 40
    for eng in engine_with({}):
        if entry == "checksum_batchv":
            def call():
                small = [dict(data=inp.bytes, n=1000, stride=64, seg_len=64), dict(data=inp.bytes, n=1000, stride=40, seg_len=40)]
                return eng.checksum_batchv(small + [dict(data=inp.bytes, n=n_alone, offsets=off),
                                                    dict(data=inp.bytes, n=500, stride=1500, seg_len=1500)])
        else:
            def call():
                small = [dict(dgrams=inp.bytes, n=1000, stride=40, dgram_len=40),
                         dict(dgrams=inp.bytes, n=500, stride=1500, dgram_len=1500)]
                outs = eng.ipv4_tcp_batchv(small + [dict(dgrams=inp.bytes, n=n_alone, offsets=off),
                                                    dict(dgrams=inp.bytes, n=100, stride=4000, dgram_len=4000)], 1)
                return [t for o in outs for t in o]
        rows, outs = _traced(eng, torch, [call] * 3)
        _same(outs, entry)
    return rows


def trace_refresh():
    inp = inputs()
    off = inp.offsets("uniform", REFRESH_N)
    for eng in engine_with({}):
        rows, outs = _traced(eng, inp.torch,
                             [lambda: _call(eng, inp, "checksum_batch", REFRESH_N, off, 0)] * REFRESH_CALLS)
        _same(outs, "refresh")
    return rows


def trace_evict():
    inp = inputs()
    bufs = [inp.offsets("uniform", EVICT_N).clone() for _ in range(5)]
    for eng in engine_with({}):
        calls = [lambda b=bufs[j]: _call(eng, inp, "checksum_batch", EVICT_N, b, 0) for j in EVICT_SEQ]
        rows, outs = _traced(eng, inp.torch, calls)
        _same(outs, "evict")
    return rows


def trace_group(group):
    """{case key: rows} of one group"""
    keys = group_keys()[group]
    out = {}
    for key in keys:
        entry, mix, n, force = key.split("|")
        if group.startswith("batchv-"):
            out[key] = trace_batchv(entry, int(n))
        elif group == "refresh":
            out[key] = trace_refresh()
        elif group == "evict":
            out[key] = trace_evict()
        else:
            out[key] = trace_single(entry, mix, int(n), force)
    return out


# ---- the tests --------------------------------------------------------------
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_every_case():
    """no GPU: the fixture has exactly the cases this module runs, and says
    which commit they were recorded on"""
    fx = _fixture()
    want = {k for keys in group_keys().values() for k in keys}
    assert set(fx["cases"]) == want, sorted(set(fx["cases"]) ^ want)[:10]
    assert len(fx["commit"]) == 40 and int(fx["commit"], 16) >= 0


@pytest.fixture(scope="module")
def shared_inputs():
    global _inputs
    yield inputs()
    _inputs.close()
    _inputs = None


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(group_keys()))
def test_dispatch_trace(shared_inputs, group):
    fx = _fixture()["cases"]
    got = trace_group(group)
    for key, rows in got.items():
        print(key, rows[:3])
        assert key in fx, f"{key}: not in {FIXTURE}"
        assert rows == fx[key], f"{key}: {rows[:3]} != recorded {fx[key][:3]}"
    if group == "refresh":
        # kPlanRefresh = 64: the miss asks for the plan, then every 64th lookup of the key
        (rows,) = got.values()
        assert [c + 1 for c, r in enumerate(rows) if r[6]] == [1, 65, 129], rows
        assert [r[4:6] for r in rows[1:]] == [[1, 0]] * (REFRESH_CALLS - 1)
    if group == "evict":
        # kPlanSlots = 4, least recently used out: the model's hits and misses
        (rows,) = got.values()
        lru, want = [], []
        for b in EVICT_SEQ:
            want.append([1, 0] if b in lru else [0, 1])
            if b in lru:
                lru.remove(b)
            lru = (lru + [b])[-4:]
        assert [r[4:6] for r in rows] == want, rows


def _record():
    import subprocess

    if "--commit" in sys.argv:  # a tree without its history
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    cases = {}
    for group in sorted(group_keys()):
        cases.update(trace_group(group))
        print(group, flush=True)
    inputs().close()
    with open(out, "w") as f:
        f.write('{"commit": "%s",\n "cases": {\n' % commit)
        f.write(",\n".join("  %s: %s" % (json.dumps(k), json.dumps(cases[k])) for k in sorted(cases)))
        f.write("\n }}\n")
    print(f"recorded {len(cases)} cases on {commit} -> {out}")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/test_gpu_dispatch_trace.py --record [--out FILE] [--commit HASH]")
    _record()
