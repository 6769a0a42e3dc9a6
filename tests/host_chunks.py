"""A model of the host-memory pipeline's chunking and the inputs that walk it
(pure numpy, no GPU).

icsum_host.cpp cuts a host batch into chunks that fit a staging slot, by
bytes (`slot_bytes`) and by count (kSlotSegs, kWrapSlotSegs for the wraps),
rebases each chunk to the aligned base of its slot, lets the 2..kMaxSlots
slots take turns, sends a segment longer than a slot through as slot-sized
pieces of kSubPiece sub-pieces, and scatters the results back at retire.
`plan()` restates the contract of that cutting — greedy, maximal — without
looking at the code; the generators below build batches whose plans put a
cut, a slot turn or a piece edge on every case that arithmetic has, and the
`classes` helpers say which of them a batch reaches, so tests/test_host_chunks.py
can prove the coverage from the inputs alone and tests/test_gpu_host_chunks.py
can tie the model to the engine through ics_dispatch_info's chunk counters.
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc")


def _const(path, name):
    """`constexpr T name = V;` / `= T(V) << K;` of a source file, read as text"""
    with open(os.path.join(CSRC, path)) as f:
        text = f.read()
    m = re.findall(r"constexpr\s+\w+\s+" + name + r"\s*=\s*(?:\w+\((\d+)\)|(\d+))(?:\s*<<\s*(\d+))?\s*;", text)
    assert len(m) == 1, (path, name, m)
    a, b, sh = m[0]
    return int(a or b) << int(sh or 0)


K_SLOT_SEGS = _const("icsum_ctx.h", "kSlotSegs")
K_WRAP_SLOT_SEGS = _const("icsum_ctx.h", "kWrapSlotSegs")
K_MAX_SLOTS = _const("icsum_ctx.h", "kMaxSlots")
K_SUB_PIECE = _const("icsum_host.cpp", "kSubPiece")

SLOT_MB = 1  # ICSUM_HOST_SLOT_MB of the swept engines
S = SLOT_MB << 20
NSLOTS = (2, 3, 4)  # ICSUM_HOST_SLOTS of the swept engines: the least, the default, kMaxSlots
ZERO_COPY_MAX = 2 << 20  # ics_ctx::zero_copy_max's default
GUARD = 5  # sentinel elements kept past n in every output array

Chunk = namedtuple("Chunk", "i0 i1 b0 b1 piece pos last")


# ---------------------------------------------------------------- model ----
def plan(n, spec, slot_bytes, cap_n, allow_pieces):
    """The chunks of a host batch of n segments: `spec` is the n + 1 offsets
    or (stride, seg_len).  Greedy and maximal: a chunk starts at the first
    segment not yet taken and takes segments while they are at most cap_n and
    the bytes from its first segment's start to its last segment's end are at
    most slot_bytes.  A segment longer than a slot is taken alone, as pieces
    of slot_bytes (the last one the rest): chunks (i, i + 1, b0, b1, True,
    pos, last) with pos the piece's offset inside the segment.  Raises
    ValueError for such a segment when pieces are not allowed (the fused IPv4
    kernel and the wraps)."""
    if isinstance(spec, tuple):
        stride, seg_len = spec
        start = lambda i: i * stride  # noqa: E731
        end = lambda i: i * stride + seg_len  # noqa: E731
    else:
        off = [int(x) for x in spec] if n < 4096 else None
        arr = np.asarray(spec, dtype=np.uint64).astype(np.int64)
        start = (lambda i: off[i]) if off else (lambda i: int(arr[i]))  # noqa: E731
        end = (lambda i: off[i + 1]) if off else (lambda i: int(arr[i + 1]))  # noqa: E731
    out = []
    i = 0
    while i < n:
        b0 = start(i)
        if end(i) - b0 > slot_bytes:
            if not allow_pieces:
                raise ValueError(f"segment {i} exceeds the slot")
            L = end(i) - b0
            for pos in range(0, L, slot_bytes):
                take = min(slot_bytes, L - pos)
                out.append(Chunk(i, i + 1, b0 + pos, b0 + pos + take, True, pos, pos + take == L))
            i += 1
            continue
        hi = min(n, i + cap_n)  # at most cap_n segments
        if isinstance(spec, tuple):
            j = i + 1
            if stride == 0:
                j = hi
            else:
                j = min(hi, i + (slot_bytes - seg_len) // stride + 1)
        else:
            # ends are non-decreasing: the last segment whose end is within the slot
            j = i + int(np.searchsorted(arr[i + 1:hi + 1], b0 + slot_bytes, side="right"))
        assert j > i
        out.append(Chunk(i, j, b0, end(j - 1), False, 0, False))
        i = j
    return out


def counters(chunks, zero_copy_max=ZERO_COPY_MAX):
    """(host_zero_copy, host_dma_chunks) a call with this plan adds: a batch in
    one whole chunk of at most zero_copy_max bytes is read in place, every
    other chunk is DMA'd"""
    if len(chunks) == 1 and not chunks[0].piece and chunks[0].b1 - chunks[0].b0 <= zero_copy_max:
        return 1, 0
    return 0, len(chunks)


def offsets_of(lens, lead=0):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    return off + np.uint64(lead)


# -------------------------------------------------------- offsets batches --
def _frozen(lens):
    """an int64 array no test can change (the generators' results are shared)"""
    a = np.array(lens, dtype=np.int64)
    a.setflags(write=False)
    return a


def _split(rng, total, k):
    """k positive lengths summing to total"""
    if k == 1:
        return [total]
    cuts = np.sort(rng.choice(np.arange(1, total), k - 1, replace=False))
    return np.diff(np.concatenate([[0], cuts, [total]])).tolist()


# segments per full chunk: one slot-sized segment; means of ~150 KB, 26 KB,
# 1.5 KB, 350 B and 52 B (every geometry class down to the tiny kernel)
_CHUNK_SEGS = (1, 7, 40, 700, 3000, 20000)


@functools.lru_cache(maxsize=None)
def cut_batches():
    """[(name, lens)]: offsets batches whose segments all fit a slot (every
    entry point takes them), one per chunk count of 1, nslots - 1, nslots,
    nslots + 1 and 2 nslots + 1 for nslots = 2, 3, 4.  A full chunk holds
    S - 1 bytes, S bytes, S - r bytes with the next segment r + 1 bytes (it
    would make S + 1), or one segment of S bytes exactly; the S - 1 and S - r
    payloads walk the chunk starts through the residues mod 16.  Empty
    segments stand first in a chunk (the batch's first: behind a byte cut the
    next segment is never empty), last in a chunk (behind S bytes exactly: they
    still fit) and at the end of the batch in the chunk behind the last cut."""
    rng = np.random.default_rng(0xC0C)
    counts = sorted({c for s in NSLOTS for c in (1, s - 1, s, s + 1, 2 * s + 1)})
    out = []
    t = 0
    todo = set(range(1, 16))  # chunk-start residues mod 16 not reached yet
    for count in counts:
        lens = [0] if count % 2 else []
        need = 0  # the least first segment of this chunk: what did not fit the one before
        cur = 0  # this chunk's start mod 16
        for j in range(count):
            kind = (0, 2, 1, 2, 3, 2)[(t + j) % 6]
            k = _CHUNK_SEGS[(t + 2 * j) % len(_CHUNK_SEGS)]
            head = [need] if need else []
            if j == count - 1:  # the last chunk: a part of a slot, then the batch's trailing empties
                lens += head + _split(rng, int(rng.integers(50_000, 200_000)), 9) + [0, 0]
                break
            if kind == 3:  # one segment of S bytes exactly
                pay = S
                lens += [S]
            else:
                r = min((r for r in range(1, 16) if (cur - r) % 16 in todo), default=1 + (t + j) % 15)
                pay = (S - 1, S, S - r)[kind]
                lens += head + _split(rng, pay - need, k)
                if kind == 1 or j % 2:
                    lens += [0]  # an empty segment last in the chunk
            # the next chunk's first segment: one byte more than fits, or a few
            need = S - pay + 1 + (0 if kind == 2 else (t + j) % 9)
            cur = (cur + pay) % 16
            todo.discard(cur)
        out.append((f"cut{count}", _frozen(lens)))
        t += count
    return out


@functools.lru_cache(maxsize=None)
def piece_batches():
    """[(name, lens)]: checksum-only offsets batches with segments longer than
    a slot: S + 1, 2 S, 2 S + 1 and 3 S - 1 bytes; last pieces of 1,
    kSubPiece - 1, kSubPiece and kSubPiece + 1 bytes; a pieced segment first,
    in the middle, last, and two adjacent; odd and even segment starts."""
    rng = np.random.default_rng(0xC0D)
    small = lambda k: rng.integers(0, 3000, k).tolist()  # noqa: E731
    a = [S + 1] + small(50) + [2 * S, 2 * S + 1] + small(3) + [S + K_SUB_PIECE - 1]
    b = small(30) + [3 * S - 1, 0, S + K_SUB_PIECE] + small(7) + [S + K_SUB_PIECE + 1] + small(5)
    return [("pieces_a", _frozen(a)), ("pieces_b", _frozen(b))]


def _tiny_lens(rng, k):
    """k lengths of 0..2 bytes, mean 0.45: 2^20 of them stay well below a 1 MiB slot"""
    return rng.choice(np.array([0, 1, 2]), k, p=[0.7, 0.15, 0.15]).astype(np.int64)


DGRAM_LENS = (40, 47, 60)  # the valid datagrams put on either side of a count cut
LONG_SEG = 300_000  # the long segment of a chunk whose mean length picks the tiny or small kernel


@functools.lru_cache(maxsize=None)
def count_cut_batch(cap, d, seed):
    """(lens, valid): cap + d segments of 0..2 bytes behind a run of `cap`
    empty segments — 2 cap + d in all.  The first chunk is the empty run
    (nb = 0, cut by count); the second is cut by count again, cap segments
    holding one LONG_SEG-byte segment and less than a slot in all; the d
    segments left make the third.  `valid`: the indices of 40..60-byte
    segments, to be dressed as valid datagrams: the first of the second chunk,
    its last three, and every one of the d behind the cut."""
    rng = np.random.default_rng(seed)
    core = _tiny_lens(rng, cap + d)
    core[cap // 3] = LONG_SEG
    where = [0, cap - 3, cap - 2, cap - 1] + list(range(cap, cap + d))
    for j, i in enumerate(where):
        core[i] = DGRAM_LENS[j % len(DGRAM_LENS)]
    lens = np.concatenate([np.zeros(cap, dtype=np.int64), core])
    return _frozen(lens), _frozen(np.asarray(where, dtype=np.int64) + cap)


# --------------------------------------------------- fixed-stride batches --
# (name, stride, seg_len, n, overlapping): `overlapping` batches only go
# through what reads (a writer's stores would hit its neighbours)
FIXED = [
    ("stride_eq_len", 1500, 1500, 2000, False),
    ("stride_gt_len", 600, 100, 4000, False),  # the last segment's padding is not part of its chunk
    ("stride_lt_len", 64, 1500, 33000, True),
    ("stride_1", 1, 5000, 1500, True),
    ("stride_0", 0, 1500, 3000, True),
    ("stride_gt_slot", S + 4096, 3000, 5, False),
    ("stride_gt_slot_len_eq_slot", S + 13, S, 3, False),
    ("len_0", 4096, 0, 600, False),  # chunks of S bytes exactly and no segment bytes
    ("len_0_stride_7", 7, 0, 5000, False),
    ("len_0_stride_0", 0, 0, 100, True),
]
# len > S: the checksum alone (pieces)
FIXED_PIECES = [
    ("len_gt_slot", S + 70_000, S + K_SUB_PIECE + 1, 2, False),
    ("len_gt_slot_overlapping", 1001, S + 1, 3, True),
]


def fixed_bytes(stride, seg_len, n):
    """the bytes a fixed-stride batch reaches"""
    return (n - 1) * stride + seg_len if n else 0


# ---------------------------------------------------------------- classes --
def chunk_classes(lens, chunks):
    """What the plan of an offsets batch (lengths `lens`) reaches, as a dict:
      payloads   the set of S - (chunk bytes) over the non-piece chunks that a
                 byte cut ended (0: S bytes exactly, 1: S - 1, ...)
      plus_one   a byte cut whose next segment would have made S + 1
      residues   b0 mod 16 over every chunk
      empty_first   a chunk of several segments whose first is empty
      empty_last    a chunk a byte cut ended whose last segment is empty
      empty_tail a batch ending in empty segments in a chunk behind a cut
      empty_chunk a chunk with segments and no bytes
      piece_tails the lengths of the last pieces
      piece_at   where pieced segments stand: 'first', 'middle', 'last', 'adjacent'
      count      the number of chunks"""
    lens = np.asarray(lens, dtype=np.int64)
    n = lens.size
    c = {"payloads": set(), "plus_one": False, "residues": set(), "empty_first": False, "empty_last": False,
         "empty_tail": False, "empty_chunk": False, "piece_tails": set(), "piece_at": set(), "count": len(chunks)}
    pieced = sorted({ch.i0 for ch in chunks if ch.piece})
    for i in pieced:
        c["piece_at"].add("first" if i == 0 else "last" if i == n - 1 else "middle")
        if i + 1 in pieced:
            c["piece_at"].add("adjacent")
    for k, ch in enumerate(chunks):
        c["residues"].add(ch.b0 % 16)
        nb = ch.b1 - ch.b0
        if ch.piece:
            if ch.last:
                c["piece_tails"].add(nb)
            continue
        if nb == 0:
            c["empty_chunk"] = True
        if ch.i1 < n and lens[ch.i1] <= S and nb + lens[ch.i1] > S:  # ended by a byte cut
            c["payloads"].add(S - nb)
            c["plus_one"] |= bool(nb + lens[ch.i1] == S + 1)
            c["empty_last"] |= bool(lens[ch.i1 - 1] == 0)
        c["empty_first"] |= bool(lens[ch.i0] == 0 and nb > 0)
        if k > 0 and not chunks[k - 1].piece and ch.i1 == n and lens[n - 1] == 0 and nb > 0:
            c["empty_tail"] = True
    return c


# ------------------------------------------------------------- contents ----
def fill(rng, lens, valid=()):
    """Random bytes for an offsets batch of these lengths, laid out from 0:
    every segment of >= 20 bytes starts 0x4h (version 4, a header length of
    0..15 words), every third of them has protocol 6; the segments listed in
    `valid` (40..60 bytes) are IPv4 + TCP headers that verify but for their
    checksums (IHL 5, total length right, TCP data offset 5)."""
    lens = np.asarray(lens, dtype=np.int64)
    off = offsets_of(lens).astype(np.int64)
    buf = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    at = off[:-1][lens >= 20]
    buf[at] = 0x40 | rng.integers(0, 16, at.size).astype(np.uint8)
    buf[at[::3] + 9] = 6
    for i in valid:
        s, L = int(off[i]), int(lens[i])
        buf[s], buf[s + 2], buf[s + 3], buf[s + 9], buf[s + 32] = 0x45, L >> 8, L & 255, 6, 0x50
    return buf


def inits_for(rng, n):
    """random inits with 0 and 0xFFFFFFFF among them (the first two and the last two)"""
    init = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    init[:2] = (0, 0xFFFFFFFF)[:min(n, 2)]
    init[-2:] = (0xFFFFFFFF, 0)[-min(n, 2):]
    return init


def random_msgs(rng, n):
    """n ics_tcp_msg records (engine.TCP_MSG_DTYPE), every field random"""
    from tcpip_network_protocol_stack_amd.engine import TCP_MSG_DTYPE

    m = np.zeros(n, dtype=TCP_MSG_DTYPE)
    for f, hi in (("src", 2**32), ("dst", 2**32), ("seqno", 2**32), ("ackno", 2**32), ("src_port", 2**16),
                  ("dst_port", 2**16), ("window", 2**16), ("id", 2**16)):
        m[f] = rng.integers(0, hi, n, dtype=np.uint64)
    m["flags"] = rng.choice([0x10, 0x12, 0x11, 0x14, 0x02, 0x01, 0x00, 0x17], n)
    m["ttl"] = rng.choice([128, 64, 1, 255], n)
    return m


def _be(v, k):
    """k big-endian bytes of every value: [n, k] uint8"""
    v = np.asarray(v).astype(np.uint64)
    return np.stack([(v >> np.uint64(8 * (k - 1 - j))) & np.uint64(255) for j in range(k)], axis=1).astype(np.uint8)


def header_fields(m, total_len):
    """[n, 40] uint8: the IPv4 + TCP headers serialize() lays out for records
    m and datagrams of total_len bytes (the length field wraps mod 2^16), both
    checksum fields zero (ipv4_header.cpp:113-123, tcp_segment.cpp:109-118)."""
    n = m.size
    h = np.zeros((n, 40), dtype=np.uint8)
    h[:, 0] = 0x45
    h[:, 2:4] = _be(np.asarray(total_len, dtype=np.uint64) & np.uint64(0xFFFF), 2)
    h[:, 4:6] = _be(m["id"], 2)
    h[:, 6] = 0x40
    h[:, 8] = m["ttl"]
    h[:, 9] = 6
    h[:, 12:16] = _be(m["src"], 4)
    h[:, 16:20] = _be(m["dst"], 4)
    h[:, 20:22] = _be(m["src_port"], 2)
    h[:, 22:24] = _be(m["dst_port"], 2)
    h[:, 24:28] = _be(m["seqno"], 4)
    h[:, 28:32] = _be(m["ackno"], 4)
    h[:, 32] = 0x50
    h[:, 33] = m["flags"]
    h[:, 34:36] = _be(m["window"], 2)
    return h


def wire_in_place(orc, buf, m, offsets=None, stride=0, dgram_len=0):
    """The bytes ics_tcp_wrap_batch_host leaves in `buf` (a copy is returned):
    every datagram of >= 40 bytes gets its 40 header bytes, the header fields
    written for all of them at once and both checksums by one PATCH call of
    the oracle over the batch; shorter datagrams keep their bytes."""
    n = m.size
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
        starts, lens = off[:-1], np.diff(off)
    else:
        starts, lens = np.arange(n, dtype=np.int64) * stride, np.full(n, dgram_len, dtype=np.int64)
    want = np.array(buf, dtype=np.uint8, copy=True)
    full = lens >= 40
    idx = starts[full][:, None] + np.arange(40)
    want[idx] = header_fields(m[full], lens[full])
    short = np.flatnonzero((lens >= 20) & ~full)  # PATCH would store into these: put them back
    keep = [(int(starts[i]), want[starts[i]:starts[i] + lens[i]].copy()) for i in short]
    orc.ipv4_tcp_batch(want, n, 2, offsets=offsets, stride=stride, dgram_len=dgram_len)
    for s, b in keep:
        want[s:s + b.size] = b
    return want


def wire_headers(orc, payloads, m, offsets=None, stride=0, payload_len=0):
    """The n x 40 header bytes ics_tcp_wrap_headers_host returns for these
    payloads: the datagrams are laid out with their headers (payload i behind
    40 i + 40 more bytes), patched by the oracle in one call, and the headers
    read back."""
    n = m.size
    if offsets is not None:
        off = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
        starts, lens = off[:-1], np.diff(off)
    else:
        starts, lens = np.arange(n, dtype=np.int64) * stride, np.full(n, payload_len, dtype=np.int64)
    doff = np.zeros(n + 1, dtype=np.int64)
    doff[1:] = np.cumsum(lens + 40)
    d = np.zeros(int(doff[-1]), dtype=np.uint8)
    payloads = np.asarray(payloads, dtype=np.uint8)
    big = lens >= 4096
    for i in np.flatnonzero(big):  # few: copied one by one
        d[doff[i] + 40:doff[i + 1]] = payloads[starts[i]:starts[i] + lens[i]]
    sl = np.where(big, 0, lens)
    seg = np.repeat(np.arange(n, dtype=np.int64), sl)
    within = np.arange(int(sl.sum()), dtype=np.int64) - np.repeat(np.cumsum(sl) - sl, sl)
    d[doff[seg] + 40 + within] = payloads[starts[seg] + within]
    idx = doff[:-1][:, None] + np.arange(40)
    d[idx] = header_fields(m, lens + 40)
    orc.ipv4_tcp_batch(d, n, 2, offsets=doff.astype(np.uint64))
    return d[idx].reshape(-1)
