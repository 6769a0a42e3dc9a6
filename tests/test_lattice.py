"""CPU: the lattices of tests/lattice.py reach what the GPU sweeps of
tests/test_gpu_lattice.py claim to enumerate, proven from the inputs alone
(no kernel, no oracle), and the tests' geometry tables name exactly the
instantiated kernel shapes.  If a sweep is thinned below one of these
conditions, or a new (LPS, UNROLL, MODE) is instantiated without being added
to the swept tables, a test here fails."""
import os
import re

import numpy as np
import pytest

import lattice
from conftest import ROOT
from test_gpu_parity import GEOMETRIES, SMALL_GEOMETRIES
from test_gpu_wrap import WRAP_GEOMETRIES

ALL_SHAPES = sorted({tuple(g[:3]) for g in GEOMETRIES + SMALL_GEOMETRIES + WRAP_GEOMETRIES})
_gid = lambda g: f"lps{g[0]}x{g[1]}m{g[2]}"  # noqa: E731


def _missing(hit):
    """the first few (k index, nch - kP, head chunk, start byte, tail bytes) a lattice leaves out"""
    return [(int(a), int(b) - 1, int(c), int(d), int(e) + 1) for a, b, c, d, e in np.argwhere(~hit)[:5]]


# ------------------------------------------------------- generators -------
def test_pass_lengths_window():
    got = lattice.pass_lengths(64)
    assert got == sorted(set(got)) and got[0] == 0
    assert set(range(289)) <= set(got)
    for k in (1, 2):
        assert set(range(1024 * k - 160, 1024 * k + 33)) <= set(got)
    assert max(got) == 2048 + 32 and max(lattice.pass_lengths(64, extra=60)) == 2048 + 92
    assert lattice.pass_lengths(4) == list(range(289))  # the small shapes' windows lie inside 0..288
    assert max(lattice.pass_lengths(512, ks=(1,))) == 8192 + 32


def test_overlap_batch_has_no_zero_byte_and_holds_every_segment():
    buf = lattice.overlap_batch(np.random.default_rng(1), 1000)
    assert buf.dtype == np.uint8 and buf.size == 144 + 1000 + 16 and buf.min() >= 1
    assert (lattice.STARTS - 1) + 1000 <= buf.size


@pytest.mark.parametrize("lead", [0, 3, 127, 130])
def test_packed_batch_puts_target_j_at_residue_j(lead):
    lens, off = lattice.packed_batch(77, lead)
    assert lens.size == 256 and off.size == 257 and off[0] == lead
    assert (np.diff(off.astype(np.int64)) == lens).all()
    assert (lens[1::2] == 77).all() and (lens[0::2] < 128).all() and (lens >= 0).all()
    assert (off[1:-1:2].astype(np.int64) % 128 == np.arange(128)).all()
    lens, off = lattice.packed_batch([5, 0, 9], 3, [17, 17, 2])
    assert lens.tolist() == [14, 5, 123, 0, 113, 9] and off[1::2].astype(np.int64).tolist()[:3] == [17, 145, 258]


def test_group_classes_against_a_plain_loop():
    rng = np.random.default_rng(5)
    s = rng.integers(0, 300, 400)
    e = s + rng.integers(0, 1200, 400)
    for P, anchor in ((4, 16), (32, 128)):
        want = np.zeros((2, 3, anchor // 16, 16, 16), dtype=bool)
        for a, b in zip(s.tolist(), e.tolist()):
            if b <= a:
                continue
            a0 = a - a % anchor
            nch = -(-(b - a0) // 16)
            for ki, k in enumerate((1, 2)):
                if abs(nch - k * P) <= 1:
                    want[ki, nch - k * P + 1, (a - a0) // 16, a % 16, (b - a0 - 1) % 16] = True
        assert (lattice.group_classes(P, anchor, s, e) == want).all()


# ------------------------------------------------- per-group shapes -------
@pytest.mark.parametrize("g", ALL_SHAPES, ids=_gid)
def test_stride1_lattice_hits_every_class(g):
    """every (head chunk, start byte, tail bytes) at nch = kP - 1, kP, kP + 1
    for k = 1, 2: 8 x 16 x 16 classes on the line grid, 16 x 16 on the
    16-byte grid, at each of the six nch"""
    P, anchor = lattice.geometry_P(g), lattice.geometry_anchor(g)
    hit = lattice.stride1_classes(P, anchor, lattice.pass_lengths(P))
    assert hit.shape == (2, 3, anchor // 16, 16, 16)
    assert hit.all(), _missing(hit)


@pytest.mark.parametrize("g", ALL_SHAPES, ids=_gid)
def test_stride1_lattice_of_the_ipv4_sweep(g):
    """the fused kernel sums from 20..60 bytes into the datagram (4 x IHL):
    with the window widened by 60 the summed range meets every class too, at
    the shortest and the longest header"""
    P, anchor = lattice.geometry_P(g), lattice.geometry_anchor(g)
    for lo in (20, 60):
        hit = lattice.stride1_classes(P, anchor, lattice.pass_lengths(P, extra=60), lo=lo)
        assert hit.all(), (lo, _missing(hit))


@pytest.mark.parametrize("g", sorted(set(WRAP_GEOMETRIES)), ids=_gid)
def test_stride1_lattice_of_the_wrap_sweep(g):
    """the headers-apart wrap sweeps the k = 1 window only"""
    P, anchor = lattice.geometry_P(g), lattice.geometry_anchor(g)
    L = lattice.wrap_lengths(P)
    assert set(range(49)) <= set(L) and set(L) <= set(lattice.pass_lengths(P, ks=(1,)))
    hit = lattice.stride1_classes(P, anchor, L, ks=(1,))
    assert hit.all(), _missing(hit)


def test_thinned_stride1_lattice_would_be_noticed():
    # one length short of the window, or starts in one line only without its
    # neighbour's first chunk: classes go missing
    L = lattice.pass_lengths(64)
    assert not lattice.stride1_classes(64, 128, [x for x in L if x != 1024 - 158]).all()
    assert not lattice.stride1_classes(64, 128, L, n=127).all()
    assert not lattice.stride1_classes(4, 16, [x for x in L if x != 18]).all()


def test_packed_lattice_hits_every_class_of_the_twoclass_long_path():
    P = lattice.TWOCLASS_LONG_P
    assert P == 112
    L = lattice.twoclass_lengths()
    assert set(range(97)) <= set(L)  # the short / long split
    hit = lattice.packed_classes(P, 128, L, lead=3)
    assert hit.all(), _missing(hit)
    for lo in (20, 60):  # the fused kernel's TCP part, at the shortest and the longest header
        hit = None
        for x in lattice.twoclass_lengths(60):
            off = lattice.packed_batch(x, 3)[1].astype(np.int64)
            h = lattice.group_classes(P, 128, np.minimum(off[:-1] + lo, off[1:]), off[1:])
            hit = h if hit is None else hit | h
        assert hit.all(), (lo, _missing(hit))


# ------------------------------------------------------------ k_span ------
@pytest.fixture(scope="module")
def span_offsets():
    return [off for _, off in lattice.span_batches()]


def test_span_points_against_a_plain_loop():
    _, off = lattice.span_batches()[37]
    o = [int(x) for x in off]
    for S in (1, 7, 63):
        A, B = lattice.span_points(S, off)
        k = j = 0
        for i0 in range(0, len(o) - 1, S):
            m = min(S, len(o) - 1 - i0)
            a0 = o[i0] // 128 * 128
            nch = -(-(o[i0 + m] - a0) // 16) if o[i0 + m] > a0 else 0
            for p in range(m + 1):
                pc = (o[i0 + p] - a0) // 16
                assert (A["span"][k], A["window"][k], A["chunk"][k], A["byte"][k], bool(A["past"][k])) == \
                    (i0 // S, pc // 256, pc % 256, o[i0 + p] % 16, pc >= nch)
                k += 1
                if p < m and o[i0 + p + 1] - o[i0 + p] >= 40:
                    assert (B["window_a"][j], B["window_b"][j]) == (pc // 256, (o[i0 + p] + 40 - a0) // 16 // 256)
                    j += 1
        assert k == A["span"].size and j == B["span"].size


@pytest.mark.parametrize("S", lattice.SPAN_SIZES)
def test_span_lattice_pins_every_window_edge(span_offsets, S):
    """an A point in chunk 255 of window w - 1 and in chunk 0 of window w at
    every byte 0..15 for w = 1..4; spans whose last offset sits on the aligned
    end of their last chunk; for S = 7 and 63 an in-place wrap's B point in
    another window than its A point, the A point in a window of each index
    mod 3 (with S = 1 every span starts in its own first line: B cannot
    straddle)"""
    edge = np.zeros((5, 2, 16), dtype=bool)  # [w, chunk 255 of w - 1 | chunk 0 of w, byte]
    past = False
    straddle = set()
    for off in span_offsets:
        A, B = lattice.span_points(S, off)
        for side, chunk in ((0, 255), (1, 0)):
            sel = A["chunk"] == chunk
            w = A["window"][sel] + (1 - side)
            ok = (w >= 1) & (w <= 4)
            edge[w[ok], side, A["byte"][sel][ok]] = True
        past |= bool(A["past"].any())
        straddle |= {int(a) % 3 for a, b in zip(B["window_a"], B["window_b"]) if a != b}
    assert edge[1:].all(), np.argwhere(~edge[1:])[:5].tolist()
    assert past
    if S == 1:
        assert not straddle
    else:
        assert straddle == {0, 1, 2}


def test_span_lattice_fills_the_grid_stride_form(span_offsets):
    # {"span_segs": 7, "span_blocks": 5}: more spans than 5 blocks of 4 waves hold
    for off in span_offsets:
        assert -(-(off.size - 1) // 7) > 5 * 4


def test_span_lattice_is_small():
    assert sum(int(off[-1]) for _, off in lattice.span_batches()) < 16 << 20


# --------------------------------------------------- geometry tables ------
def _table(name):
    with open(os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc", "kernels", "icsum_common.h")) as f:
        text = f.read()
    m = re.search(r"#define\s+" + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", text)
    assert m, name
    rows = re.findall(r"X\(([^)]*)\)", m.group(1))
    assert rows and "X(" + ") X(".join(rows) + ")" == " ".join(m.group(1).replace("\\\n", " ").split())
    return [tuple({"true": 1, "false": 0}.get(v.strip(), v.strip()) for v in r.split(",")) for r in rows]


def test_geometry_tables_name_exactly_the_instantiations():
    """ICS_GEOMETRIES / ICS_SMALL_GEOMETRIES of kernels/icsum_common.h, read as
    text: WRAP_GEOMETRIES is the (LPS, UNROLL, MODE) list itself; GEOMETRIES
    the same with the tiny kernel (1, 4, mode 4) where the checksum has no
    (1, 4, mode 0) shape; SMALL_GEOMETRIES the small-segment table."""
    inst = [(int(l), int(u), int(m)) for l, u, _, m in _table("ICS_GEOMETRIES")]
    assert len(set(inst)) == len(inst)
    assert sorted(WRAP_GEOMETRIES) == sorted(inst) and len(WRAP_GEOMETRIES) == len(inst)
    assert (1, 4, 0) in inst
    assert sorted(GEOMETRIES) == sorted((1, 4, 4) if g == (1, 4, 0) else g for g in inst)
    assert len(GEOMETRIES) == len(inst)
    small = [(int(l), int(u), 0, int(k)) for l, u, k in _table("ICS_SMALL_GEOMETRIES")]
    assert sorted(SMALL_GEOMETRIES) == sorted(small) and len(SMALL_GEOMETRIES) == len(small)
