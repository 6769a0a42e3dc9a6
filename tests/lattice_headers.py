"""The per-item shape surface of k_frame and k_tcp_unwrap, enumerated (the
header kernels' counterpart of lattice.py).

Both kernels load a frame / datagram as the aligned 16-byte blocks that hold
it, one dwordx4 per lane, clamped at the item's last block, and parse from the
item's start dword on.  An item's shape is therefore (start residue mod 16) x
(blocks held) x (clamped or not) and, for a datagram, the header length (the
options path loads the TCP header from start + 4 hlen, at any residue mod 4)
and the data offset.  The family suites reach that where random length mixes
land; here it is laid out by construction:

  targets   every length class x every start residue 0..15; a datagram's
            (hlen, data offset) pair walks all 12 combinations along the
            residues, offset by the length class, so that every class meets
            every pair, and both option-carrying header lengths meet every
            TCP start residue mod 4
  batches   packed offsets; a pad item of 0..15 bytes before each target puts
            it on its residue (pads are items too, of random bytes: never a
            datagram, at most a bare Ethernet header); batch b holds every
            target, rotated so that target 3 b is the last one and ends at
            the allocation's last byte — a third of the targets, in turn

test_shape_lattice_headers.py proves these claims from the inputs alone."""
import random

import numpy as np

FRAME_LENGTHS = [13, 14, 15, 29, 30, 33, 34, 35, 41, 42, 43, 46, 47, 50, 60]
DGRAM_LENGTHS = [19, 20, 39, 40, 41, 43, 44, 47, 48, 59, 60, 61, 79, 80]
HLENS, DOFFS = [5, 6, 15], [4, 5, 6, 15]
PAIRS = [(h, d) for h in HLENS for d in DOFFS]


def _frame_class_ok(L, frames, ins):
    """the 16 frames of one length class show every class that length can: not for us, IPv4 and ARP for us, a
    parsing datagram from 34 bytes, a parsing ARP message from 42"""
    from frame_ref import FR_ARP, FR_ARP_OK, FR_DGRAM, FR_FOR_US, FR_IPV4, classify
    from test_gpu_frames import MACS

    st = [classify(f, MACS[k]) for f, k in zip(frames, ins)]
    need = [] if L < 14 else [FR_FOR_US, FR_IPV4, FR_ARP] + ([FR_DGRAM] if L >= 34 else []) + ([FR_ARP_OK] if L >= 42 else [])
    return 0 in st and all(any(x & bit for x in st) for bit in need)


def frame_targets(seed=0x1A77):
    """(frames, ingress interfaces, residues): 15 x 16 targets of test_gpu_frames' classes.  Each length class
    takes the first seed from `seed` on whose 16 draws show every class that length can (_frame_class_ok)."""
    from test_gpu_frames import make_frame

    frames, ins, res = [], [], []
    for L in FRAME_LENGTHS:
        for s in range(seed, seed + 1000):
            rng = np.random.default_rng([s, L])
            ks = [int(rng.integers(0, 4)) for _ in range(16)]
            fs = [make_frame(rng, L, k) for k in ks]
            if _frame_class_ok(L, fs, ks):
                break
        else:
            raise AssertionError(f"no seed gives every class at length {L}")
        frames += fs
        ins += ks
        res += list(range(16))
    return frames, np.array(ins, np.uint32), np.array(res)


def _dgram_class_ok(L, dgrams, shape):
    """the 16 datagrams of one length class hold, for every header length whose TCP header fits, one that parses
    with that header length, and one that does not parse"""
    from unwrap_ref import PARSED, verify_status

    ok = [verify_status(d) & PARSED == PARSED for d in dgrams]
    fits = [h for h in HLENS if 4 * h + 20 <= L]
    return not all(ok) and all(any(p and d[0] & 15 == h and s[0] == h for p, d, s in zip(ok, dgrams, shape))
                               for h in fits)


def dgram_targets(seed=0x1A78):
    """(datagrams, residues, (hlen, doff) per target): 14 x 16 targets; seeds chosen as in frame_targets"""
    from unwrap_ref import make_dgram

    dgrams, res, shape = [], [], []
    for c, L in enumerate(DGRAM_LENGTHS):
        sh = [PAIRS[(r + 5 * c) % len(PAIRS)] for r in range(16)]
        for s in range(seed, seed + 1000):
            rng = random.Random(s * 131 + L)
            ds = [make_dgram(rng, L, h, d, fix=0.9, flip=0.05) for h, d in sh]
            if _dgram_class_ok(L, ds, sh):
                break
        else:
            raise AssertionError(f"no seed gives every class at length {L}")
        dgrams += ds
        res += list(range(16))
        shape += sh
    return dgrams, np.array(res), shape


def n_batches(n_targets):
    return -(-n_targets // 3)


def batch(targets, residues, b, seed=0):
    """Batch b: (items, offsets n + 1, index of each item's target or -1 for a pad).  The targets from 3 b + 1
    on, then those up to 3 b, each behind a pad that puts it on its residue; the allocation is the items' bytes
    and nothing more."""
    rng = random.Random(seed * 7919 + b)
    n = len(targets)
    order = [(3 * b + 1 + k) % n for k in range(n)]
    items, which, pos = [], [], 0
    for t in order:
        pad = (int(residues[t]) - pos) % 16
        items.append(rng.randbytes(pad))
        which.append(-1)
        items.append(targets[t])
        which.append(t)
        pos += pad + len(targets[t])
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return items, off, np.array(which)


def blocks_held(start, length):
    """aligned 16-byte blocks that hold [start, start + length)"""
    return ((start + length - 1) >> 4) - (start >> 4) + 1 if length else 0
