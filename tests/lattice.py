"""Enumerated inputs for the alignment / pass-boundary sweeps (pure numpy, no GPU).

Every summing routine cuts a segment into 16-byte chunks on a grid anchored
on the 16-byte block or the 128-byte line that holds the first byte; a lane
group covers P = LPS x UNROLL chunks per pass and loops over longer segments.
With nch = the chunks the group walks for one segment (head-line chunks
included), the off-by-one surface is (head chunk 0..7) x (start byte 0..15) x
(tail bytes 1..16) x (nch in {kP - 1, kP, kP + 1}).  The generators here reach
that surface on purpose; the `classes` helpers say which of it a batch hits,
so tests/test_lattice.py can prove, from the inputs alone, that the GPU sweeps
of tests/test_gpu_lattice.py leave none of it out.

  stride-1 batches   the C-ABI allows overlapping segments (segment i =
                     bytes[i * stride, i * stride + seg_len)): stride 1 puts
                     144 consecutive segments at 144 consecutive addresses, so
                     one uploaded buffer and one call per length cover every
                     start residue mod 128 (and 16 starts in the next line);
  packed batches     for the offsets-only launches and everything that writes:
                     disjoint segments, a pad before each target so that target
                     j starts at residue j of its line;
  span lattices      packed batches whose points fall on both sides of the
                     4 KiB window edges of k_span, per span size.
"""
import numpy as np

STARTS = 144  # stride-1 segments per batch: residues 0..127 and 16 starts in the next line
WIN_CHUNKS = 256  # k_span's window: 4 KiB
SPAN_SIZES = (1, 7, 63)  # the forced span sizes the sweeps run
TWOCLASS_LONG_P = 16 * 7  # the two-class launches' long path: 16 lanes x 7 loads on the line grid


def geometry_P(g):
    """chunks one pass of a lane group covers: LPS x UNROLL"""
    return g[0] * g[1]


def geometry_anchor(g):
    """the chunk grid's anchor in bytes: the 128-byte line (mode 3) or the 16-byte block"""
    return 128 if g[2] == 3 else 16


def pass_lengths(P, extra=0, ks=(1, 2)):
    """Every length 0..288 and, for each k, every length of
    [16 k P - 160, 16 k P + 32 + extra]: with starts at every residue mod 128
    these put nch on kP - 1, kP and kP + 1 at every head chunk, start byte and
    tail.  `extra` widens the window for operations whose summed range starts
    past the segment start (IPv4: 20..60 bytes in; the in-place wrap: 40)."""
    out = set(range(0, 289))
    for k in ks:
        out.update(range(max(0, 16 * k * P - 160), 16 * k * P + 32 + extra + 1))
    return sorted(out)


def wrap_lengths(P):
    """the headers-apart wrap's sweep: payloads of 0..48 bytes and the k = 1 window"""
    return [L for L in pass_lengths(P, ks=(1,)) if L <= 48 or L >= 16 * P - 160]


def twoclass_lengths(extra=0):
    """the two-class sweeps: 0..96 (the short / long split: 4 chunks for the
    checksum, 64 bytes for IPv4), then the long path's windows around
    16 x 112 x k"""
    P = TWOCLASS_LONG_P
    return [L for L in pass_lengths(P, extra=extra) if L <= 96 or L >= 16 * P - 160]


def overlap_batch(rng, Lmax, n=STARTS):
    """One buffer of n + Lmax + 16 bytes drawn from 1..255 (no zero byte: a
    dropped or doubled byte always changes a sum) for stride-1 batches of n
    segments of up to Lmax bytes."""
    return rng.integers(1, 256, n + Lmax + 16, dtype=np.uint8)


def packed_batch(L, lead, residues=range(128)):
    """Disjoint segments: a pad of (r - cur) mod 128 bytes, then a target of L
    bytes (an int, or one length per target) that so starts at residue r of
    its line, for each r of `residues`.  Pads are ordinary segments.  Returns
    (the 2 len(residues) lengths, their n + 1 offsets from `lead`)."""
    res = np.asarray(list(residues), dtype=np.int64)
    tl = np.broadcast_to(np.asarray(L, dtype=np.int64), res.shape)
    lens = np.empty(2 * res.size, dtype=np.int64)
    cur = int(lead)
    for j in range(res.size):
        pad = (int(res[j]) - cur) % 128
        lens[2 * j], lens[2 * j + 1] = pad, tl[j]
        cur += pad + int(tl[j])
    off = np.zeros(lens.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    off += np.uint64(lead)
    return lens, off


# ------------------------------------------------------------ classes -----
def group_classes(P, anchor, starts, ends, ks=(1, 2)):
    """The (k, head chunk, start byte, tail bytes) classes segments
    [starts[i], ends[i]) hit at each nch - kP of {-1, 0, +1}: a boolean array
    [k index, nch - kP + 1, head chunk (anchor / 16), start byte 16, tail 16]."""
    s = np.asarray(starts, dtype=np.int64).ravel()
    e = np.asarray(ends, dtype=np.int64).ravel()
    keep = e > s
    s, e = s[keep], e[keep]
    a0 = s & ~np.int64(anchor - 1)
    nch = (e - a0 + 15) >> 4
    hc, sb, tail = (s - a0) >> 4, s & 15, ((e - a0 - 1) & 15)
    hit = np.zeros((len(ks), 3, anchor // 16, 16, 16), dtype=bool)
    for ki, k in enumerate(ks):
        d = nch - k * P
        ok = (d >= -1) & (d <= 1)
        hit[ki, d[ok] + 1, hc[ok], sb[ok], tail[ok]] = True
    return hit


def stride1_classes(P, anchor, lengths, n=STARTS, lo=0, ks=(1, 2)):
    """group_classes of the stride-1 batches of every length of `lengths`;
    `lo` = where the summed range starts inside the segment (0: the checksum)."""
    i = np.arange(n, dtype=np.int64)[None, :]
    L = np.asarray(lengths, dtype=np.int64)[:, None]
    return group_classes(P, anchor, np.minimum(i + lo, i + L), i + L, ks)


def packed_classes(P, anchor, lengths, lead, residues=range(128), ks=(1, 2)):
    """group_classes of packed_batch(L, lead, residues) over every L of `lengths`"""
    hit = None
    for L in lengths:
        _, off = packed_batch(L, lead, residues)
        h = group_classes(P, anchor, off[:-1].astype(np.int64), off[1:].astype(np.int64), ks)
        hit = h if hit is None else hit | h
    return hit


def span_points(S, off, lo_shift=40):
    """k_span's view of an offsets batch: spans of S segments (i0 = span x S),
    each with its windows anchored on the line of its first byte (a0c =
    (off[i0] >> 7) << 3).  Returns two dicts of equal-length arrays:
      A  every point off[i0 .. i0 + m]: span, window, chunk in the window,
         byte, past (the point sits on the aligned end of the span's last
         chunk: pc >= nch);
      B  for every segment of >= lo_shift bytes the second point lo = start +
         lo_shift (the in-place wrap): span, window_a and window_b."""
    off = np.asarray(off, dtype=np.int64)
    n = off.size - 1
    A = {k: [] for k in ("span", "window", "chunk", "byte", "past")}
    B = {k: [] for k in ("span", "window_a", "window_b")}
    for span in range((n + S - 1) // S):
        i0 = span * S
        m = min(S, n - i0)
        x = off[i0:i0 + m + 1]
        a0c = (int(x[0]) >> 7) << 3
        tend = int(x[-1])
        nch = ((tend + 15) >> 4) - a0c if tend > (a0c << 4) else 0
        pc = (x >> 4) - a0c
        A["span"].append(np.full(m + 1, span))
        A["window"].append(pc // WIN_CHUNKS)
        A["chunk"].append(pc % WIN_CHUNKS)
        A["byte"].append(x & 15)
        A["past"].append(pc >= nch)
        has = (x[1:] - x[:-1]) >= lo_shift
        qc = ((x[:-1][has] + lo_shift) >> 4) - a0c
        B["span"].append(np.full(int(has.sum()), span))
        B["window_a"].append(pc[:-1][has] // WIN_CHUNKS)
        B["window_b"].append(qc // WIN_CHUNKS)
    return ({k: np.concatenate(v) for k, v in A.items()}, {k: np.concatenate(v) for k, v in B.items()})


# ------------------------------------------------------- span lattice -----
SPAN_LEAD = 3
SPAN_WINDOWS = (1, 2, 3, 4)  # window 3 and later use each of the three register sets a second time
SPAN_TARGETS = 8  # long targets per batch
SPAN_SHORT = 66  # short targets behind them: more spans of 7 than a 5-block grid holds


def span_lattice():
    """The packed batches of the span sweeps, as a list of (target lengths,
    residues) for packed_batch(lengths, SPAN_LEAD, residues): one batch per
    window edge w = 1..4 and t = 0..31, thinned from "every length of
    [4096 k - 160, 4096 k + 32] at 128 residues" to what the window edges need.

    A span's windows start on the line of its first byte, and the first span
    of a batch starts at SPAN_LEAD whatever the span size, so the batch's
    first target (at residue r0 >= SPAN_LEAD of line 0) ends in chunk
    (r0 + L) >> 4 of that span.  With L = 4096 w - 16 + t - r0 that point sits
    in chunk 255 of window w - 1 (t < 16) or chunk 0 of window w, at byte
    t & 15.  The pad behind it is a segment of 41..45 bytes that starts on
    that point: for t < 16 its start + 40 (the in-place wrap's second point)
    lies in the next window.  The last long target ends on a 16-byte boundary,
    and SPAN_SHORT targets of 0..65 bytes follow, so that the batch has more
    spans of 7 than the capped grid of the grid-stride sweep holds and spans
    of every size end on the aligned end of their last chunk.
    tests/test_lattice.py checks all of this with span_points, not by this
    reasoning."""
    out = []
    for w in SPAN_WINDOWS:
        for t in range(32):
            r0 = 16 * (t % 8) + 3 + (5 * t + w) % 13
            L = 4096 * w - 16 + t - r0
            res = [r0, (r0 + L + 41 + t % 5) % 128] + [(r0 + 37 * j) % 128 for j in range(2, SPAN_TARGETS - 1)]
            res.append((-L) % 16 + 16 * (t % 8))
            lens = [L] * SPAN_TARGETS + list(range(SPAN_SHORT))
            res += [(11 * j + t) % 128 for j in range(SPAN_SHORT)]
            out.append((lens, res))
    return out


def span_batches():
    """(lengths, offsets) of every batch of span_lattice()"""
    return [packed_batch(L, SPAN_LEAD, res) for L, res in span_lattice()]
