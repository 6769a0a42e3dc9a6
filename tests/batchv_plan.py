"""A model of the multi-batch launches (ics_checksum_batchv / ics_ipv4_tcp_batchv)
and the inputs of their sweep (pure Python + numpy, no GPU).

A multi-batch call sorts its batches by kernel shape (BvClass), skips the empty
ones and issues one launch per group of up to kMaxBatchv batches whose grids
together hold at most kMaxBlocks blocks; a batch of more than kMaxBlocks / 4
blocks runs alone through the single-batch path (run_batchv, icsum_dispatch.cpp).
Inside a launch the grid is the concatenation of the batches' grids: block blk
belongs to the batch j with block0[j] <= blk < block0[j] + nblk[j] and runs the
class body as block blk - block0[j] of nblk[j] (kernels/icsum_batchv.h).  The
arithmetic that can be off by one: the per-class segments per block
(batchv_blocks), the block-to-batch search, the group cuts and the class edges.

  the model        cls_checksum / cls_ipv4 (the class of a descriptor), blocks
                   (its grid) and plan (the launches of a call, the batches that
                   run alone, the class ics_dispatch_info reports); every
                   constant is read as text from the sources (constants()), so a
                   change there changes the model and tests/test_batchv_plan.py
                   says which claim of the sweep no longer holds;
  the generators   the calls tests/test_gpu_batchv_sweep.py runs, as host-side
                   specs (dicts: buf, lead, stride, seg_len, n, offsets, init);
                   tests/test_batchv_plan.py proves from these inputs alone what
                   they cover.

A descriptor (`desc`) is a dict with n, stride, seg_len (the datagram length for
the fused entry), offsets (anything true: an offsets batch) and base (the byte
address of the batch mod 16).
"""
import os
import re

import numpy as np

import lattice

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tcpip_network_protocol_stack_amd",
                    "csrc")


def _text(*rel):
    with open(os.path.join(CSRC, *rel)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text, re.S)
    assert len(m) == 1, (what, len(m))
    return m[0]


def constants():
    """What the model needs, parsed from the sources:
      classes      {name: value} of enum BvClass
      per          {class value: segments per block} of batchv_blocks
      max_batchv   kMaxBatchv
      max_blocks   run_batchv's kMaxBlocks; alone_div: a batch of more than
                   max_blocks / alone_div blocks runs alone
      table_limit  bv_table accepts grids below this
      tiny_max     kTinyMaxAvg
      steps        pick_geometry's rows [(chunks or None for the last, lps, unroll, mode, segs)]
      offsets_hint avg_len_hint of an offsets batch (the checksum entry)
      dense_len    the one length the multi-batch call takes as dense
      dense_lens   dense_supported's lengths
      line64_from  lanes per segment from which a line grid runs the 64-lane body
    """
    launch_h = _text("kernels", "icsum_launch.h")
    batchv_h = _text("kernels", "icsum_batchv.h")
    checksum_h = _text("kernels", "icsum_checksum.h")
    dispatch = _text("icsum_dispatch.cpp")
    c = {}
    enum = _one(r"enum BvClass : int \{([^}]*)\}", launch_h, "BvClass")
    c["classes"] = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(","))}
    c["max_batchv"] = int(_one(r"constexpr int kMaxBatchv = (\d+);", launch_h, "kMaxBatchv"))
    c["tiny_max"] = int(_one(r"constexpr uint32_t kTinyMaxAvg = (\d+);", launch_h, "kTinyMaxAvg"))
    mode_tiny = int(_one(r"constexpr int kModeTiny = (\d+);", launch_h, "kModeTiny"))
    # batchv_blocks: "cls == A || cls == B ? 256 : cls == C ? 128 : ... : 4"
    expr = _one(r"uint64_t batchv_blocks\(int cls, uint64_t n\) \{.*?const uint64_t per = (.*?);", batchv_h, "per")
    arms = [a.strip() for a in " ".join(expr.split()).split(":")]
    per, named = {}, set()
    for arm in arms[:-1]:
        cond, value = arm.split("?")
        names = re.findall(r"cls == (\w+)", cond)
        assert names and " ".join(cond.split()) == " || ".join(f"cls == {x}" for x in names), arm
        for name in names:
            per[c["classes"][name]] = int(value)
            named.add(name)
    rest = set(c["classes"]) - named
    assert len(rest) == 1, rest  # the last arm serves exactly one class
    per[c["classes"][rest.pop()]] = int(arms[-1])
    c["per"] = per
    assert re.search(r"return \(n \+ per - 1\) / per;", batchv_h)
    c["table_limit"] = 1 << int(_one(r"return blocks < \(uint64_t\(1\) << (\d+)\);", batchv_h, "bv_table's limit"))
    sh, minus = _one(r"constexpr uint64_t kMaxBlocks = \(uint64_t\(1\) << (\d+)\) - (\d+);", dispatch, "kMaxBlocks")
    c["max_blocks"] = (1 << int(sh)) - int(minus)
    c["alone_div"] = int(_one(r"if \(nb > kMaxBlocks / (\d+)\) \{", dispatch, "the alone rule"))
    _one(r"if \(m == icsum::kMaxBatchv \|\| blocks \+ nb > kMaxBlocks\)\s+if \(int rc = flush\(\)\) return rc;",
         dispatch, "the flush rule")
    _one(r"cls\[j\] = b\[j\]\.n \? cls_of\(b\[j\]\) : -1;", dispatch, "empties are skipped")
    _one(r"for \(int c = 0; c <= icsum::kBvLane1; \+\+c\) \{", dispatch, "classes in enum order")
    _one(r"report_launch\(ctx, ICS_K_BATCHV, last_cls, int\(k\)\);", dispatch, "the report")
    # pick_geometry
    body = _one(r"Geometry pick_geometry\(uint64_t avg_len\) \{(.*?)\n\}", checksum_h, "pick_geometry")
    _one(r"const uint64_t m = \(avg_len \+ 15\) / 16;", body, "chunks")
    tiny = _one(r"if \(avg_len <= kTinyMaxAvg\) return \{(\d+), (\d+), (?:true|false), kModeTiny, (\d+)\};", body, "tiny")
    c["tiny_geometry"] = (int(tiny[0]), int(tiny[1]), mode_tiny, int(tiny[2]))
    steps = [(int(m), int(l), int(u), int(mo), int(s)) for m, l, u, mo, s in
             re.findall(r"if \(m <= (\d+)\) return \{(\d+), (\d+), (?:true|false), (\d+), (\d+)\};", body)]
    last = _one(r"\n  return \{(\d+), (\d+), (?:true|false), (\d+), (\d+)\};", body, "the last row")
    steps.append((None,) + tuple(int(x) for x in last))
    assert body.count("return") == len(steps) + 1
    assert [s[0] for s in steps[:-1]] == sorted(s[0] for s in steps[:-1])
    c["steps"] = steps
    c["offsets_hint"] = int(_one(r"return offsets \? (\d+) : seg_len;", dispatch, "avg_len_hint"))
    # the class choices
    c["dense_len"] = int(_one(r"if \(!x\.offsets && x\.seg_len == (\d+) && icsum::dense_supported\(sp\)\) "
                              r"return icsum::kBvDense64;", dispatch, "the dense class"))
    dense = _one(r"bool dense_supported\(const SegSpec& sp\) \{(.*?)\n\}", checksum_h, "dense_supported")
    _one(r"if \(sp\.offsets \|\| sp\.n == 0 \|\| sp\.stride != sp\.seg_len\) return false;", dense, "dense: stride")
    _one(r"if \(\(reinterpret_cast<uintptr_t>\(sp\.bytes\) & 15\) != 0\) return false;", dense, "dense: base")
    c["dense_lens"] = sorted(int(x) for x in re.findall(r"sp\.seg_len == (\d+)", dense))
    assert dispatch.count("if (g.mode == icsum::kModeTiny) return icsum::kBvTiny;") == 1
    assert dispatch.count("if (g.segs > 1) return icsum::kBvSmall;") == 1
    assert dispatch.count("if (g.mode == icsum::kModeTiny) return icsum::kBvLane1;") == 1
    assert dispatch.count("if (x.offsets) return icsum::kBvLine16;") == 1
    lines = re.findall(r"return g\.lps >= (\d+) \? icsum::kBvLine64 : icsum::kBvLine16;", dispatch)
    assert len(lines) == 2 and lines[0] == lines[1]
    c["line64_from"] = int(lines[0])
    assert dispatch.count("icsum::pick_geometry(avg_len_hint(x.offsets, x.seg_len))") == 1
    assert dispatch.count("icsum::pick_geometry(x.dlen)") == 1
    return c


C = constants()
DENSE, TINY, SMALL, LINE16, LINE64, LANE1 = (C["classes"][k] for k in
                                             ("kBvDense64", "kBvTiny", "kBvSmall", "kBvLine16", "kBvLine64", "kBvLane1"))
NAMES = {DENSE: "dense", TINY: "tiny", SMALL: "small", LINE16: "line16", LINE64: "line64", LANE1: "lane1"}
ENTRY_CLASSES = {"checksum": (DENSE, TINY, SMALL, LINE16, LINE64), "ipv4": (LANE1, LINE16, LINE64)}
PAIRS = [(e, c) for e in ("checksum", "ipv4") for c in ENTRY_CLASSES[e]]  # the eight (entry, class) pairs
pair_id = lambda p: f"{p[0]}-{NAMES[p[1]]}"  # noqa: E731


# ------------------------------------------------------------- the model ---
def pick_geometry(avg_len):
    """(lps, unroll, mode, segs) of pick_geometry(avg_len)"""
    if avg_len <= C["tiny_max"]:
        return C["tiny_geometry"]
    m = (avg_len + 15) // 16
    for limit, *g in C["steps"]:
        if limit is None or m <= limit:
            return tuple(g)


def _line_class(g):
    return LINE64 if g[0] >= C["line64_from"] else LINE16


def cls_checksum(desc):
    if (not desc["offsets"] and desc["seg_len"] == C["dense_len"] and desc["n"] and desc["stride"] == desc["seg_len"]
            and desc["base"] % 16 == 0 and desc["seg_len"] in C["dense_lens"]):
        return DENSE
    g = pick_geometry(C["offsets_hint"] if desc["offsets"] else desc["seg_len"])
    if g == C["tiny_geometry"]:
        return TINY
    if g[3] > 1:
        return SMALL
    return _line_class(g)


def cls_ipv4(desc):
    if desc["offsets"]:
        return LINE16
    g = pick_geometry(desc["seg_len"])
    if g == C["tiny_geometry"]:
        return LANE1
    return _line_class(g)


CLS_OF = {"checksum": cls_checksum, "ipv4": cls_ipv4}


def per_block(cls):
    return C["per"][cls]


def blocks(cls, n):
    per = C["per"][cls]
    return (n + per - 1) // per


def plan(descs, entry):
    """(launches, alone, last_lps) of one call: launches = [(class, [indices
    into descs, in slot order])] in issue order, alone = the indices that run
    through the single-batch path, last_lps = the class ics_dispatch_info
    reports in `lps` (None: no multi-batch launch, the report is another
    call's); `unroll` reports len(descs)."""
    cls = [CLS_OF[entry](d) if d["n"] else -1 for d in descs]
    launches, alone, last = [], [], None
    for c in range(LANE1 + 1):
        group, total = [], 0
        for j, d in enumerate(descs):
            if cls[j] != c:
                continue
            nb = blocks(c, d["n"])
            if nb > C["max_blocks"] // C["alone_div"]:
                alone.append(j)
                continue
            if group and (len(group) == C["max_batchv"] or total + nb > C["max_blocks"]):
                launches.append((c, group))
                group, total = [], 0
            group.append(j)
            total += nb
        if group:
            launches.append((c, group))
    if launches:
        last = launches[-1][0]
    return launches, alone, last


def block_table(cls, ns):
    """bv_table's block0[] / nblk[] of one launch"""
    nblk = [blocks(cls, n) for n in ns]
    block0 = [sum(nblk[:j]) for j in range(len(ns))]
    return block0, nblk


def find(block0, blk):
    """bv_find: the entries 1.. at or below blk (the padding is never)"""
    return sum(1 for q in range(1, len(block0)) if blk >= block0[q])


SIM_SENTINEL = 0x5A5A
MUTATIONS = ("search_gt", "lb_plus_1", "lb_minus_1", "pad_zero", "blocks_short")


def simulate(cls, ns, wants, mutation=None):
    """One launch, block by block, as k_checksum_batchv / k_ipv4_batchv run it:
    the table of bv_table, every block of the concatenated grid through
    bv_find, then the class body as block lb of nb of the batch found — the
    dense body owns segments [per lb, per lb + per), every other body walks
    blocks lb, lb + nb, ... of per segments.  A segment the body reaches gets
    its batch's expected value wants[j][seg]; everything else keeps
    SIM_SENTINEL.  `mutation` puts one off-by-one into that arithmetic:
      search_gt     bv_find compares blk > block0[q]
      lb_plus_1 / lb_minus_1   the block's index inside its batch, one off (uint32)
      pad_zero      block0[] behind the last batch is 0, not 0xFFFFFFFF
      blocks_short  batchv_blocks rounds down (at least one block)
    Descriptors behind the last batch are zero (n = 0), as bv_table leaves them."""
    per, k, cap = per_block(cls), len(ns), C["max_batchv"]
    if mutation == "blocks_short":
        nblk = [max(1, n // per) for n in ns]
        block0 = [sum(nblk[:j]) for j in range(k)]
    else:
        block0, nblk = block_table(cls, ns)
    table = block0 + [0 if mutation == "pad_zero" else 0xFFFFFFFF] * (cap - k)
    outs = [np.full(n, SIM_SENTINEL, dtype=np.int64) for n in ns]
    for blk in range(sum(nblk)):
        if mutation == "search_gt":
            j = sum(1 for q in range(1, cap) if blk > table[q])
        else:
            j = find(table, blk)
        if j >= k:
            continue  # a zero descriptor: no segments
        lb = (blk - block0[j] + {"lb_plus_1": 1, "lb_minus_1": -1}.get(mutation, 0)) & 0xFFFFFFFF
        step = per if cls == DENSE else nblk[j] * per
        g0 = lb * per
        while g0 < ns[j]:
            outs[j][g0:g0 + per] = wants[j][g0:g0 + per]
            if cls == DENSE:
                break
            g0 += step
    return outs


# ------------------------------------------------------------ the inputs ---
def desc(spec):
    return dict(n=spec["n"], stride=spec["stride"], seg_len=spec["seg_len"], offsets=spec["offsets"] is not None,
                base=spec["lead"] % 16 if spec["offsets"] is None else 0)


EMPTY = dict(buf=None, lead=0, stride=0, seg_len=0, n=0, offsets=None, init=None)

# each class's lengths in the block-edge calls (fixed lengths in bytes)
LENGTHS = {TINY: (1, 40, 56), SMALL: (57, 144, 145, 272), LINE16: (273, 1500, 2240), LINE64: (2241, 3521, 9000),
           DENSE: (64,), LANE1: (40, 56)}


def edge_sizes(per):
    """batch sizes on every side of a block edge, for one and for two blocks"""
    return [1, per - 1, per, per + 1, 2 * per - 1, 2 * per, 2 * per + 1]


def fixed_datagrams(orc, rng, n, L):
    """n datagrams of exactly L bytes as an (n, L) array: random bytes under
    mostly well-formed headers (version, header length 0..15, total length,
    protocol, TCP data offset, each sometimes wrong), every third one carrying
    the oracle's checksums"""
    d = rng.integers(0, 256, (n, L), dtype=np.uint8)
    if L >= 20 and n:
        hlen = rng.choice([5, 5, 5, 5, 6, 8, 15, 4, 0], n)
        ver = np.where(rng.random(n) < 0.9, 4, rng.integers(0, 16, n))
        d[:, 0] = (ver << 4) | hlen
        tot = np.where(rng.random(n) < 0.85, L, rng.integers(0, 65536, n))
        d[:, 2], d[:, 3] = tot >> 8, tot & 255
        d[:, 9] = np.where(rng.random(n) < 0.9, 6, rng.integers(0, 256, n))
        t = 4 * np.maximum(hlen, 5) + 12
        rows = np.flatnonzero(t < L)
        d[rows, t[rows]] = np.where(rng.random(rows.size) < 0.85, 5, rng.integers(0, 16, rows.size)) << 4
        good = np.ascontiguousarray(d[::3]).reshape(-1)
        orc.ipv4_tcp_batch(good, (n + 2) // 3, 2, stride=L, dgram_len=L)
        d[::3] = good.reshape(-1, L)
    return d


_pool = {}


def _ack_pool(orc):
    """2048 datagrams of test_gpu_parity._random_datagrams cut or padded to 56 bytes"""
    if "ack" not in _pool:
        from test_gpu_parity import _random_datagrams

        segs = _random_datagrams(np.random.default_rng(0xACC), 2048)
        _pool["ack"] = np.frombuffer(b"".join((s + bytes(56))[:56] for s in segs), dtype=np.uint8).reshape(2048, 56)
    return _pool["ack"]


def _any_pool(orc):
    """600 datagrams of _random_datagrams as they are (0..1600 bytes), for offsets batches"""
    if "any" not in _pool:
        from test_gpu_parity import _random_datagrams

        _pool["any"] = _random_datagrams(np.random.default_rng(0xA11), 600)
    return _pool["any"]


def make_batch(orc, rng, entry, cls, n, j):
    """One batch of n segments of class cls with its own bytes; j picks the
    length of LENGTHS, the stride's slack, the lead and (checksum) whether the
    batch has inits; every fourth line64 checksum batch and line16 datagram
    batch is an offsets batch (the checksum's with empty segments)."""
    L = LENGTHS[cls][j % len(LENGTHS[cls])]
    lead = 0 if cls == DENSE else (0, 1, 0, 5)[(j // 2) % 4]
    stride = L if cls == DENSE else L + (0, 0, 3, 8)[j % 4]
    init = None
    if entry == "checksum" and j % 2:
        init = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    if j % 4 == 3 and (entry, cls) in (("checksum", LINE64), ("ipv4", LINE16)):
        if entry == "checksum":
            lens = rng.choice([0, 0, 1, 40, 41, 1500, 3000], n)
            segs = [rng.integers(0, 256, int(x), dtype=np.uint8).tobytes() for x in lens]
        else:
            pool = _any_pool(orc)
            segs = [pool[i] for i in rng.choice(len(pool), n)]
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in segs])
        off += np.uint64(lead + 2)
        buf = np.frombuffer(b"\xa5" * (lead + 2) + b"".join(segs) + b"\0" * 16, dtype=np.uint8).copy()
        return dict(buf=buf, lead=0, stride=0, seg_len=0, n=n, offsets=off, init=init)
    if entry == "checksum":
        rows = rng.integers(0, 256, (n, L), dtype=np.uint8)
    elif cls == LANE1:  # half from _random_datagrams, half of exactly L bytes
        pool = _ack_pool(orc)
        rows = np.concatenate([pool[rng.choice(2048, n - n // 2, replace=False), :L],
                               fixed_datagrams(orc, rng, n // 2, L)])[rng.permutation(n)]
    else:
        rows = fixed_datagrams(orc, rng, n, L)
    buf = np.full(lead + n * stride + 16, 0xA5, dtype=np.uint8)
    body = buf[lead:lead + n * stride].reshape(n, stride)
    body[:, :L] = rows
    body[:, L:] = rng.integers(0, 256, (n, stride - L), dtype=np.uint8)
    return dict(buf=buf, lead=lead, stride=stride, seg_len=L, n=n, offsets=None, init=init)


_calls = {}


def _cached(key, make):
    if key not in _calls:
        _calls[key] = make()
    return _calls[key]


def edge_calls(orc, entry, cls):
    """Seven calls of 16 batches: call r has edge_sizes(per)[(r + s) % 7]
    segments in slot s, so every size stands once in slot 0 and once in slot
    15, and the one-block sizes 1, per - 1, per stand side by side."""
    def make():
        rng = np.random.default_rng(0xED6E00 + 16 * cls + (entry == "ipv4"))
        sizes = edge_sizes(per_block(cls))
        return [[make_batch(orc, rng, entry, cls, sizes[(r + s) % 7], r + s) for s in range(C["max_batchv"])]
                for r in range(7)]
    return _cached(("edge", entry, cls), make)


CUT_KS = (1, 2, 15, 16, 17, 31, 32, 33)


def cut_call(orc, entry, cls, k):
    """k batches of one class, 1 .. 2 per + 1 segments each"""
    def make():
        rng = np.random.default_rng(0xC0700 + 1000 * k + 16 * cls + (entry == "ipv4"))
        per = per_block(cls)
        return [make_batch(orc, rng, entry, cls, int(rng.integers(1, 2 * per + 2)), j) for j in range(k)]
    return _cached(("cut", entry, cls, k), make)


def mixed_call(orc, entry):
    """About 100 descriptors: the entry's classes in turn (more than 16 batches
    of each), an empty batch first, last and after every eleventh"""
    def make():
        rng = np.random.default_rng(0x313ED + (entry == "ipv4"))
        classes = ENTRY_CLASSES[entry]
        out = [dict(EMPTY)]
        for j in range(95 if entry == "checksum" else 96):
            cls = classes[j % len(classes)]
            out.append(make_batch(orc, rng, entry, cls, int(rng.integers(1, 2 * per_block(cls) + 2)),
                                  j // len(classes)))
            if j % 11 == 10:
                out.append(dict(EMPTY))
        out.append(dict(EMPTY))
        return out
    return _cached(("mixed", entry), make)


def _fixed(orc, rng, entry, L, n, stride=None, lead=0):
    stride = L if stride is None else stride
    rows = rng.integers(0, 256, (n, L), dtype=np.uint8) if entry == "checksum" else fixed_datagrams(orc, rng, n, L)
    buf = np.full(lead + n * stride + 16, 0xA5, dtype=np.uint8)
    body = buf[lead:lead + n * stride].reshape(n, stride)
    body[:, :L] = rows
    body[:, L:] = 0x3C
    init = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32) if entry == "checksum" else None
    return dict(buf=buf, lead=lead, stride=stride, seg_len=L, n=n, offsets=None, init=init)


EDGE_N = 301  # segments of a class-edge batch: more than one block of every class, the last one partial


def class_edge_cases(orc):
    """[(id, entry, spec, the class the issue's table names)]: one batch each"""
    def make():
        rng = np.random.default_rng(0xC1A55)
        out = []
        for L, cls in ((56, TINY), (57, SMALL), (272, SMALL), (273, LINE16), (2240, LINE16), (2241, LINE64)):
            out.append((f"checksum-{L}", "checksum", _fixed(orc, rng, "checksum", L, EDGE_N), cls))
        out.append(("checksum-64-aligned", "checksum", _fixed(orc, rng, "checksum", 64, EDGE_N), DENSE))
        out.append(("checksum-64-base1", "checksum", _fixed(orc, rng, "checksum", 64, EDGE_N, lead=1), SMALL))
        out.append(("checksum-64-stride72", "checksum", _fixed(orc, rng, "checksum", 64, EDGE_N, stride=72), SMALL))
        out.append(("checksum-32-dense-shaped", "checksum", _fixed(orc, rng, "checksum", 32, EDGE_N), TINY))
        out.append(("checksum-128-dense-shaped", "checksum", _fixed(orc, rng, "checksum", 128, EDGE_N), SMALL))
        for L, cls in ((56, LANE1), (57, LINE16), (2240, LINE16), (2241, LINE64)):
            out.append((f"ipv4-{L}", "ipv4", _fixed(orc, rng, "ipv4", L, EDGE_N), cls))
        out.append(("checksum-offsets", "checksum", make_batch(orc, rng, "checksum", LINE64, EDGE_N, 3), LINE64))
        out.append(("ipv4-offsets", "ipv4", make_batch(orc, rng, "ipv4", LINE16, EDGE_N, 3), LINE16))
        return out
    return _cached("class_edges", make)


# the bodies behind a table: (lps, unroll, chunk-grid anchor in bytes) of each
# class's body in k_checksum_batchv / k_ipv4_batchv and the passes swept
BODY = {SMALL: (4, 2, 16, (1, 2)), LINE16: (16, 8, 128, (1,)), LINE64: (64, 8, 128, (1, 2))}


def table_lengths(cls):
    """Lists of 16 lengths (one stride-1 batch of lattice.STARTS segments
    each) per call: every length the one-lane classes admit, and for the
    others the 32 lengths [B - 24, B + 8) around each pass boundary B = 16 k
    LPS UNROLL bytes inside the class's range."""
    if cls in (TINY, LANE1):
        L = list(range(C["tiny_max"] + 1))
        L += L[:-len(L) % 16]
    else:
        lps, unroll, _, ks = BODY[cls]
        L = [x for k in ks for x in range(16 * k * lps * unroll - 24, 16 * k * lps * unroll + 8)]
    return [L[i:i + 16] for i in range(0, len(L), 16)]


TABLE_LMAX = max(max(max(c) for c in table_lengths(cls)) for cls in (TINY, SMALL, LINE16, LINE64))


def table_buffer(nibble5):
    """lattice.overlap_batch for the longest table length (nibble5: about half
    of the bytes read as a header length of 5, for the fused entry)"""
    rng = np.random.default_rng(0x7AB1E + nibble5)
    buf = lattice.overlap_batch(rng, TABLE_LMAX)
    if nibble5:
        k = rng.random(buf.size) < 0.5
        buf[k] = (buf[k] & 0xF0) | 5
    return buf


# the block budget: line64 checksum batches of stride 0
BUDGET_LEN = 3521


def budget_n():
    """the largest batch that still shares a launch: four of them fill one to max_blocks - 3"""
    return per_block(LINE64) * (C["max_blocks"] // C["alone_div"])


def budget_desc(n):
    return dict(n=n, stride=0, seg_len=BUDGET_LEN, offsets=False, base=0)


# --------------------------------------------------------- expectations ----
def expect(orc, entry, spec, mode=0):
    """checksum: the u16 values; ipv4: (ip_ck, tcp_ck, status, the buffer after the call)"""
    n = spec["n"]
    if entry == "checksum":
        if spec["offsets"] is not None:
            return orc.checksum_batch(spec["buf"], n, offsets=spec["offsets"], init=spec["init"])
        return orc.checksum_batch(spec["buf"][spec["lead"]:], n, stride=spec["stride"], seg_len=spec["seg_len"],
                                  init=spec["init"])
    after = spec["buf"].copy()
    if spec["offsets"] is not None:
        ip, tcp, st = orc.ipv4_tcp_batch(after, n, mode, offsets=spec["offsets"])
    else:
        ip, tcp, st = orc.ipv4_tcp_batch(after[spec["lead"]:], n, mode, stride=spec["stride"],
                                         dgram_len=spec["seg_len"])
    return ip, tcp, st, after
