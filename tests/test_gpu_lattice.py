"""GPU: every start alignment and pass boundary through each kernel shape.

The lattices of tests/lattice.py (whose coverage tests/test_lattice.py proves
on the CPU) run through every forced kernel shape and the default dispatch,
bit-exact against the oracle:

  stride-1 sweeps   one buffer uploaded once, 144 overlapping segments at
                    consecutive addresses, one call per length: the checksum
                    (u16 values, raw sums with carried parity; again under the
                    bounds-checked build), the fused IPv4/TCP kernel's
                    read-only modes and the headers-apart wrap, per shape; the
                    default dispatch around each geometry threshold;
  packed sweeps     disjoint segments, target j at residue j of its line, for
                    the offsets-only launches (two-class, binned) and for
                    everything that writes (PATCH, in-place wrap, both router
                    forms): the whole buffer is compared afterwards;
  span sweeps       the window-edge lattice through k_span at span sizes 1, 7,
                    63 and the grid-stride form.

Every input is valid (monotone offsets, segments inside their allocation).
A reference depends on the length (or batch) alone — the buffers, inits and
records are the same for every shape — so it is computed once and shared by
all the cases.  A failure names (shape, length, segment, start residue)."""
import ctypes

import numpy as np
import pytest

import lattice
from conftest import engine_with, force_id
from test_gpu_parity import GEOMETRIES, SMALL_GEOMETRIES, _t, _u16, _u32
from test_gpu_twoclass import _sentinel
from test_gpu_wrap import WRAP_GEOMETRIES

pytestmark = pytest.mark.gpu

N1 = lattice.STARTS
_KEYS = ("lps", "unroll", "mode", "segs")


def _gid(g):
    return f"lps{g[0]}x{g[1]}m{g[2]}" + (f"s{g[3]}" if len(g) > 3 else "")


def _ran(eng, kernel, lps=None, unroll=None, tag=""):
    """the forced launch is the one that ran (an uninstantiated shape would
    fall back to the default and sweep nothing new)"""
    info = eng.dispatch_info()
    assert info["kernel"] == kernel, (tag, info)
    if lps is not None:
        assert (info["lps"], info["unroll"]) == (lps, unroll), (tag, info)


def _fail(tag, what, L, i, start, got, want):
    pytest.fail(f"{tag} {what}: length {L}, segment {i}, start residue {int(start) % 128}: "
                f"got {int(got):#x}, want {int(want):#x}")


def _cmp_rows(tag, what, lengths, got, want, start_of=lambda j, i: i):
    """got / want: [length index, segment]"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if bad.size:
        j, i = (int(v) for v in bad[0])
        _fail(f"{tag} ({bad.shape[0]} wrong)", what, lengths[j], i, start_of(j, i), got[j, i], want[j, i])


def _rows(n_rows, n, dtype):
    """sentinel-filled outputs, one row per call: an output no kernel writes shows up"""
    import torch

    if dtype == torch.uint8:
        return torch.full((n_rows, n), 0x5A, dtype=dtype, device="cuda:0")
    return _sentinel(n_rows * n, dtype).view(n_rows, n)


def _msgs(rng, n):
    from test_gpu_wrap import _random_batch

    return _random_batch(rng, n, fixed=1)[1]


def _wrap_fields(m, total):
    """[n, 40] header bytes as serialize(wrap_tcp_in_ip(msg)) lays them out,
    both checksum fields zero (test_gpu_wrap._oracle_wire, vectorised);
    `total`: each datagram's length (its 16-bit field wraps)"""
    n = m.size
    h = np.zeros((n, 40), dtype=np.uint8)
    be = lambda v, k: np.stack([(np.asarray(v, dtype=np.uint64) >> np.uint64(8 * (k - 1 - b))) & np.uint64(255)  # noqa: E731
                                for b in range(k)], axis=1).astype(np.uint8)
    h[:, 0], h[:, 6], h[:, 9], h[:, 32] = 0x45, 0x40, 6, 0x50
    h[:, 2:4] = be(np.asarray(total, dtype=np.uint64) & np.uint64(0xFFFF), 2)
    h[:, 4:6], h[:, 8] = be(m["id"], 2), m["ttl"]
    h[:, 12:16], h[:, 16:20] = be(m["src"], 4), be(m["dst"], 4)
    h[:, 20:22], h[:, 22:24] = be(m["src_port"], 2), be(m["dst_port"], 2)
    h[:, 24:28], h[:, 28:32] = be(m["seqno"], 4), be(m["ackno"], 4)
    h[:, 33], h[:, 34:36] = m["flags"], be(m["window"], 2)
    return h


# ============================================================ stride 1 =====
LMAX1 = 16 * 2 * 512 + 32 + 60  # the longest length a stride-1 sweep runs (64 x 8, k = 2, IPv4's window)


class _Overlap:
    """One stride-1 buffer on the host and the device, the per-segment words,
    and the references by length (shared by every case of the module)."""

    def __init__(self, orc, seed, nibble5=False):
        rng = np.random.default_rng(seed)
        self.orc = orc
        self.buf = lattice.overlap_batch(rng, LMAX1)
        if nibble5:  # about half of the bytes read as IHL 5: the speculated s + 20 stream
            k = rng.random(self.buf.size) < 0.5  # and the options re-sum both run at every alignment
            self.buf[k] = (self.buf[k] & 0xF0) | 5
        assert self.buf.min() >= 1
        self.init = rng.integers(0, 2**32, N1, dtype=np.uint64).astype(np.uint32)
        self.odd = rng.integers(0, 2, N1).astype(np.uint8)
        self.msgs = _msgs(rng, N1)
        self.d, self.dinit, self.dodd = _t(self.buf), _t(self.init), _t(self.odd)
        self.dmsgs = _t(self.msgs.view(np.uint8).copy())
        self.ref = {}

    def want(self, op, L):
        key = (op, L)
        if key not in self.ref:
            o, b = self.orc, self.buf
            if op == "csum":
                r = o.checksum_batch(b, N1, stride=1, seg_len=L, init=self.init)
            elif op == "sum":
                r = o.sum_batch(b, N1, stride=1, seg_len=L, init=self.init, odd=self.odd)
            elif op in ("ipv4_0", "ipv4_1"):
                c = b.copy()
                r = o.ipv4_tcp_batch(c, N1, int(op[-1]), stride=1, dgram_len=L)
                assert (c == b).all()
            else:  # "apart": the 40 header bytes of header + payload i, both checksums by the oracle's PATCH
                w = np.empty((N1, 40 + L), dtype=np.uint8)
                w[:, :40] = _wrap_fields(self.msgs, np.full(N1, 40 + L))
                w[:, 40:] = np.lib.stride_tricks.sliding_window_view(b, L)[:N1] if L else 0
                w = w.reshape(-1)
                st = o.ipv4_tcp_batch(w, N1, 2, stride=40 + L, dgram_len=40 + L)[2]
                assert (st & 3 == 3).all()
                r = w.reshape(N1, 40 + L)[:, :40].copy()
            self.ref[key] = r
        return self.ref[key]


@pytest.fixture(scope="module")
def ov(orc):
    return _Overlap(orc, 0x1A77)


@pytest.fixture(scope="module")
def ov4(orc):
    return _Overlap(orc, 0x1A74, nibble5=True)


def _sweep_checksum(eng, ov, lengths, tag, ran, sums_only=False):
    import torch

    o16 = None if sums_only else _rows(len(lengths), N1, torch.int16)
    o32 = _rows(len(lengths), N1, torch.int32)
    for j, L in enumerate(lengths):
        if not sums_only:
            eng.checksum_batch(ov.d, n=N1, stride=1, seg_len=L, init=ov.dinit, out=o16[j])
            ran(eng, (tag, L))
        eng.sum_batch(ov.d, n=N1, stride=1, seg_len=L, init=ov.dinit, odd=ov.dodd, out=o32[j])
        ran(eng, (tag, L))
    if not sums_only:
        _cmp_rows(tag, "checksum", lengths, _u16(o16), [ov.want("csum", L) for L in lengths])
    _cmp_rows(tag, "sum", lengths, _u32(o32), [ov.want("sum", L) for L in lengths])


def _sweep_ipv4_readonly(eng, ov4, lengths, mode, tag, ran):
    import torch

    ip, tcp = _rows(len(lengths), N1, torch.int16), _rows(len(lengths), N1, torch.int16)
    st = _rows(len(lengths), N1, torch.uint8)
    for j, L in enumerate(lengths):
        eng.ipv4_tcp_batch(ov4.d, mode, n=N1, stride=1, dgram_len=L, ip_ck=ip[j], tcp_ck=tcp[j], status=st[j])
        ran(eng, (tag, L))
    want = [ov4.want(f"ipv4_{mode}", L) for L in lengths]
    _cmp_rows(tag, f"mode {mode} ip_ck", lengths, _u16(ip), [w[0] for w in want])
    _cmp_rows(tag, f"mode {mode} tcp_ck", lengths, _u16(tcp), [w[1] for w in want])
    _cmp_rows(tag, f"mode {mode} status", lengths, st.cpu().numpy(), [w[2] for w in want])
    assert (ov4.d.cpu().numpy() == ov4.buf).all(), (tag, "the device buffer changed")


# ------------------------------------------------- checksum, per shape ----
@pytest.fixture(scope="module", params=[(g, d) for d in (False, True) for g in GEOMETRIES + SMALL_GEOMETRIES],
                ids=lambda p: _gid(p[0]) + ("-debug" if p[1] else ""))
def shape_eng(request):
    g, debug = request.param
    for eng in engine_with(dict(zip(_KEYS, g)), debug=debug):
        eng.shape, eng.debug = g, debug
        yield eng


def test_checksum_every_shape(shape_eng, ov):
    """pass_lengths(P) at 144 consecutive starts: checksum_batch and
    sum_batch (random inits, random carried parity); under the bounds-checked
    build (every ICS_CHECK16 envelope meets every edge: a load outside the
    segment's blocks fails the call) the raw sums"""
    g = shape_eng.shape
    kernel = "tiny" if g[2] == 4 else ("small" if len(g) > 3 else "checksum")
    _sweep_checksum(shape_eng, ov, lattice.pass_lengths(lattice.geometry_P(g)), _gid(g),
                    lambda e, t: _ran(e, kernel, g[0], g[1], t), sums_only=shape_eng.debug)


# --------------------------------------------------- default dispatch -----
def _threshold_lengths():
    out = set()
    for m in (5, 9, 17, 56, 69, 82, 120, 140, 220):  # pick_geometry's steps, in chunks
        out.update(range(16 * m - 16, 16 * m + 17))
    for c in (56, 1664):  # kTinyMaxAvg; ipv4_fixed_geometry's limit
        out.update(range(max(0, c - 16), c + 17))
    return sorted(out)


def test_default_dispatch_around_every_threshold(engine, ov, ov4):
    """parity only: which shape runs on either side of a threshold stays the
    dispatch's choice"""
    L = _threshold_lengths()
    _sweep_checksum(engine, ov, L, "auto", lambda e, t: None)
    for mode in (0, 1):
        _sweep_ipv4_readonly(engine, ov4, L, mode, "auto", lambda e, t: None)


# ------------------------------------ fused IPv4, read-only, per shape ----
@pytest.fixture(scope="module", params=WRAP_GEOMETRIES, ids=_gid)
def ipv4_shape_eng(request):
    # every shape ipv4_geometry can produce: the (LPS, UNROLL, MODE) table itself
    for eng in engine_with(dict(zip(_KEYS, request.param))):
        eng.shape = request.param
        yield eng


@pytest.mark.parametrize("mode", [0, 1], ids=["compute", "verify"])
def test_ipv4_readonly_every_shape(ipv4_shape_eng, ov4, mode):
    """pass_lengths(P, extra=60) at 144 consecutive starts; about half of the
    bytes read as IHL 5, the rest as any header length (options re-summed,
    header lengths past the datagram's end, < 5): all three outputs, and the
    device buffer unchanged"""
    g = ipv4_shape_eng.shape
    _sweep_ipv4_readonly(ipv4_shape_eng, ov4, lattice.pass_lengths(lattice.geometry_P(g), extra=60), mode, _gid(g),
                         lambda e, t: _ran(e, "ipv4", g[0], g[1], t))


# ----------------------------------- headers-apart wrap, per shape --------
@pytest.fixture(scope="module", params=[(g, p) for g in WRAP_GEOMETRIES for p in (1, 2)],
                ids=lambda gp: f"{_gid(gp[0])}-passes{gp[1]}")
def wrap_shape_eng(request):
    g, passes = request.param
    for eng in engine_with({**dict(zip(_KEYS, g)), "wrap_passes": passes}):
        eng.shape, eng.passes = g, passes
        yield eng


def test_wrap_headers_apart_every_shape(wrap_shape_eng, ov):
    """stride-1 payloads of 0..48 bytes and the k = 1 window, random records:
    the 40 header bytes against the oracle's wire bytes, both checksum arrays"""
    import torch

    eng, g = wrap_shape_eng, wrap_shape_eng.shape
    tag = f"{_gid(g)} passes {eng.passes}"
    lengths = lattice.wrap_lengths(lattice.geometry_P(g))
    hd = torch.full((len(lengths), N1 * 40), 0xA5, dtype=torch.uint8, device="cuda:0")
    ip, tcp = _rows(len(lengths), N1, torch.int16), _rows(len(lengths), N1, torch.int16)
    for j, L in enumerate(lengths):
        eng.tcp_wrap_headers(ov.d, ov.dmsgs, hd[j], n=N1, stride=1, payload_len=L, ip_ck=ip[j], tcp_ck=tcp[j])
        _ran(eng, "wrap" if eng.passes == 1 else "wrap_2pass", g[0], g[1], (tag, L))
    want = np.stack([ov.want("apart", L) for L in lengths])  # [length, segment, 40]
    got = hd.cpu().numpy().reshape(len(lengths), N1, 40)
    bad = np.argwhere((got != want).any(axis=2))
    if bad.size:
        j, i = (int(v) for v in bad[0])
        pytest.fail(f"{tag} header: length {lengths[j]}, segment {i}, start residue {i % 128}: "
                    f"got {got[j, i].tobytes().hex()}, want {want[j, i].tobytes().hex()}")
    w16 = want.astype(np.uint16)
    _cmp_rows(tag, "ip_ck", lengths, _u16(ip), (w16[:, :, 10] << 8) | w16[:, :, 11])
    _cmp_rows(tag, "tcp_ck", lengths, _u16(tcp), (w16[:, :, 36] << 8) | w16[:, :, 37])
    assert (ov.d.cpu().numpy() == ov.buf).all(), (tag, "the payloads changed")


# ============================================================== packed =====
PK_LEAD = 3
PK_LMAX = 16 * 512 + 32 + 60  # the longest target of a packed sweep (64 x 8, k = 1, IPv4's window)
PK_N = 256


class _Packed:
    """One buffer for packed_batch(L, PK_LEAD) of every L, uploaded once: a
    pristine device copy restores the working buffer before each writing
    call, so a reference depends on L alone and is shared by every engine.
    Writers' references are kept as (positions, bytes) against the pristine
    buffer."""

    def __init__(self, orc, seed):
        import torch

        rng = np.random.default_rng(seed)
        self.orc = orc
        size = PK_LEAD + 128 * (127 + PK_LMAX) + 64
        self.buf = rng.integers(1, 256, size, dtype=np.uint8)
        k = rng.random(size) < 0.5
        self.buf[k] = (self.buf[k] & 0xF0) | 5
        self.init = rng.integers(0, 2**32, PK_N, dtype=np.uint64).astype(np.uint32)
        self.odd = rng.integers(0, 2, PK_N).astype(np.uint8)
        self.msgs = _msgs(rng, PK_N)
        self.d0 = _t(self.buf)
        self.d = torch.empty_like(self.d0)
        self.d.copy_(self.d0)
        self.dinit, self.dodd = _t(self.init), _t(self.odd)
        self.dmsgs = _t(self.msgs.view(np.uint8).copy())
        self.ref, self.offs = {}, {}

    def off(self, L):
        if L not in self.offs:
            off = lattice.packed_batch(L, PK_LEAD)[1]
            self.offs[L] = (off, _t(off), int(off[-1]) + 16)
        return self.offs[L]

    def restore(self):
        self.d.copy_(self.d0)

    # ---- router input: headers that forward (and some that do not) at the target starts
    def router_headers(self, L):
        """(positions, bytes): 20 header bytes per target of >= 24 bytes —
        version 4, IHL 5 (6 on every tenth), every ttl class, the reserved
        flag bit on some, a valid checksum but on every seventh"""
        off = self.off(L)[0]
        if L < 24:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint8)
        s = off[1:-1:2].astype(np.int64)
        j = np.arange(s.size)
        w = self.buf[s[:, None] + np.arange(24)].copy()
        hl = np.where(j % 10 == 0, 6, 5)
        w[:, 0] = 0x40 | hl
        w[:, 6] = np.where(j % 6 == 0, w[:, 6] | 0x80, w[:, 6] & 0x7F)
        w[:, 8] = (j * 37) % 256
        w[j % 16 == 1, 8] = 1
        w[j % 16 == 9, 8] = 0
        w[:, 10:12] = 0
        # the checksum the reference's serialize() gives these fields (the oracle's COMPUTE)
        c = self.orc.ipv4_tcp_batch(w.reshape(-1), s.size, 0, stride=24, dgram_len=24)[0].astype(np.int64)
        c = np.where(j % 7 == 3, c ^ 1, c)
        w[:, 10], w[:, 11] = c >> 8, c & 255
        return (s[:, None] + np.arange(20)).ravel(), w[:, :20].ravel()

    def _diff(self, hb, size):
        idx = np.flatnonzero(hb[:size] != self.buf[:size])
        return idx, hb[idx].copy()

    def want(self, op, L):
        key = (op, L)
        if key in self.ref:
            return self.ref[key]
        o, b = self.orc, self.buf
        off, _, size = self.off(L)
        n = off.size - 1
        if op == "csum":
            r = o.checksum_batch(b, n, offsets=off, init=self.init)
        elif op == "sum":
            r = o.sum_batch(b, n, offsets=off, init=self.init, odd=self.odd)
        elif op in ("ipv4_0", "ipv4_1", "ipv4_2"):
            hb = b[:size].copy()
            r = o.ipv4_tcp_batch(hb, n, int(op[-1]), offsets=off) + (self._diff(hb, size),)
            assert op == "ipv4_2" or r[3][0].size == 0
        elif op == "wrap":
            # fields in place where the datagram holds its 40 header bytes, then the oracle's PATCH of each
            hb = b[:size].copy()
            s, ln = off[:-1].astype(np.int64), np.diff(off.astype(np.int64))
            ok = ln >= 40
            hb[s[ok, None] + np.arange(40)] = _wrap_fields(self.msgs[ok], ln[ok])
            # PATCH writes inside its own datagram only: patch a copy of the whole batch, keep
            # the two checksum fields of the datagrams that hold their headers
            pb = hb.copy()
            ipw, tcpw, st = o.ipv4_tcp_batch(pb, n, 2, offsets=off)
            assert (st[ok] & 3 == 3).all()
            at = s[ok, None] + np.array([10, 11, 36, 37])
            hb[at] = pb[at]
            r = (np.where(ok, ipw, 0), np.where(ok, tcpw, 0), ok, self._diff(hb, size))
        else:  # "router": status, the forwarded headers (zeros where dropped), the bytes after the in-place step
            hb = b[:size].copy()
            pos, val = self.router_headers(L)
            hb[pos] = val
            before = hb.copy()
            status, hd = np.zeros(n, dtype=np.uint8), np.zeros((n, 20), dtype=np.uint8)
            f, base, stp = o.lib().orc_router_ttl, hb.ctypes.data, status.ctypes.data
            st_t = ctypes.POINTER(ctypes.c_uint8)
            for i, (a, e) in enumerate(zip(off[:-1].tolist(), off[1:].tolist())):
                f(base + a, e - a, ctypes.cast(stp + i, st_t))
            fw = np.flatnonzero(status)
            hd[fw] = hb[off[:-1].astype(np.int64)[fw, None] + np.arange(20)]
            assert L < 24 or 0 < int(status.sum()) < n
            r = (status, hd.ravel(), self._diff(before, size), self._diff(hb, size))
        self.ref[key] = r
        return r

    def expect_bytes(self, diff, size):
        w = self.buf[:size].copy()
        w[diff[0]] = diff[1]
        return w

    def put(self, diff):
        """the same few bytes into the working device buffer"""
        import torch

        if diff[0].size:
            self.d[torch.from_numpy(diff[0]).cuda()] = torch.from_numpy(diff[1]).cuda()


@pytest.fixture(scope="module")
def pk(orc):
    return _Packed(orc, 0x9AC2)


def _packed_checksum(eng, pk, lengths, tag, ran):
    import torch

    o16, o32 = _rows(len(lengths), PK_N, torch.int16), _rows(len(lengths), PK_N, torch.int32)
    for j, L in enumerate(lengths):
        _, doff, _ = pk.off(L)
        eng.checksum_batch(pk.d0, offsets=doff, init=pk.dinit, out=o16[j])
        ran(eng, (tag, L))
        eng.sum_batch(pk.d0, offsets=doff, init=pk.dinit, odd=pk.dodd, out=o32[j])
        ran(eng, (tag, L))
    start = lambda j, i: pk.off(lengths[j])[0][i]  # noqa: E731
    _cmp_rows(tag, "checksum", lengths, _u16(o16), [pk.want("csum", L) for L in lengths], start)
    _cmp_rows(tag, "sum", lengths, _u32(o32), [pk.want("sum", L) for L in lengths], start)


def _bytes_equal(tag, what, L, got, want, off):
    bad = np.flatnonzero(got != want)
    if bad.size:
        p = int(bad[0])
        i = int(np.searchsorted(off, p, side="right")) - 1
        where = f"segment {i}, start residue {int(off[i]) % 128}" if 0 <= i < off.size - 1 else "outside the batch"
        pytest.fail(f"{tag} {what}: length {L}, byte {p} ({where}; {bad.size} bytes differ): "
                    f"got {int(got[p]):#x}, want {int(want[p]):#x}")


def _packed_ipv4(eng, pk, lengths, mode, tag, ran):
    """the three outputs; the whole buffer afterwards, pads, the bytes before
    the lead and past the end included (PATCH: what the oracle wrote)"""
    import torch

    ip, tcp = _rows(len(lengths), PK_N, torch.int16), _rows(len(lengths), PK_N, torch.int16)
    st = _rows(len(lengths), PK_N, torch.uint8)
    pk.restore()
    for j, L in enumerate(lengths):
        off, doff, size = pk.off(L)
        if mode == 2:
            pk.restore()
        eng.ipv4_tcp_batch(pk.d, mode, offsets=doff, ip_ck=ip[j], tcp_ck=tcp[j], status=st[j])
        ran(eng, (tag, L))
        if mode == 2:
            _bytes_equal(tag, "PATCH bytes", L, pk.d[:size].cpu().numpy(),
                         pk.expect_bytes(pk.want("ipv4_2", L)[3], size), off)
    want = [pk.want(f"ipv4_{mode}", L) for L in lengths]
    start = lambda j, i: pk.off(lengths[j])[0][i]  # noqa: E731
    _cmp_rows(tag, f"mode {mode} ip_ck", lengths, _u16(ip), [w[0] for w in want], start)
    _cmp_rows(tag, f"mode {mode} tcp_ck", lengths, _u16(tcp), [w[1] for w in want], start)
    _cmp_rows(tag, f"mode {mode} status", lengths, st.cpu().numpy(), [w[2] for w in want], start)
    if mode == 2:
        pk.restore()
    else:
        assert (pk.d.cpu().numpy() == pk.buf).all(), (tag, "the device buffer changed")


def _packed_wrap(eng, pk, lengths, tag, ran):
    import torch

    ip, tcp = _rows(len(lengths), PK_N, torch.int16), _rows(len(lengths), PK_N, torch.int16)
    for j, L in enumerate(lengths):
        off, doff, size = pk.off(L)
        pk.restore()
        eng.tcp_wrap_batch(pk.d, pk.dmsgs, n=PK_N, offsets=doff, ip_ck=ip[j], tcp_ck=tcp[j])
        ran(eng, (tag, L))
        _bytes_equal(tag, "wrap bytes", L, pk.d[:size].cpu().numpy(), pk.expect_bytes(pk.want("wrap", L)[3], size), off)
    pk.restore()
    want = [pk.want("wrap", L) for L in lengths]
    ok = np.stack([w[2] for w in want])  # the checksum arrays where a datagram holds its headers
    start = lambda j, i: pk.off(lengths[j])[0][i]  # noqa: E731
    _cmp_rows(tag, "wrap ip_ck", lengths, np.where(ok, _u16(ip), 0), [w[0] for w in want], start)
    _cmp_rows(tag, "wrap tcp_ck", lengths, np.where(ok, _u16(tcp), 0), [w[1] for w in want], start)


def _packed_router(eng, pk, lengths, tag, apart):
    import torch

    st = _rows(len(lengths), PK_N, torch.uint8)
    hd = torch.full((len(lengths), PK_N * 20), 0xA5, dtype=torch.uint8, device="cuda:0") if apart else None
    for j, L in enumerate(lengths):
        off, doff, size = pk.off(L)
        status, _, before, after = pk.want("router", L)
        pk.restore()
        pk.put(before)
        if apart:
            eng.router_ttl_headers(pk.d, offsets=doff, hdrs=hd[j], status=st[j])
            _ran(eng, "router_hdrs", tag=(tag, L))
            _bytes_equal(tag, "router (headers apart) input", L, pk.d[:size].cpu().numpy(),
                         pk.expect_bytes(before, size), off)
        else:
            eng.router_ttl_batch(pk.d, offsets=doff, status=st[j])
            _ran(eng, "router", tag=(tag, L))
            _bytes_equal(tag, "router bytes", L, pk.d[:size].cpu().numpy(), pk.expect_bytes(after, size), off)
    pk.restore()
    want = [pk.want("router", L) for L in lengths]
    start = lambda j, i: pk.off(lengths[j])[0][i]  # noqa: E731
    _cmp_rows(tag, "router status", lengths, st.cpu().numpy(), [w[0] for w in want], start)
    if apart:
        got = hd.cpu().numpy().reshape(len(lengths), PK_N, 20)
        bad = np.argwhere((got != np.stack([w[1] for w in want]).reshape(got.shape)).any(axis=2))
        if bad.size:
            j, i = (int(v) for v in bad[0])
            pytest.fail(f"{tag} forwarded header: length {lengths[j]}, segment {i}, "
                        f"start residue {int(start(j, i)) % 128}")


# ------------------------- writers: PATCH, in-place wrap, both routers ----
# the default engine twice: at the windows of the two line-grid shapes it may pick (16 x 8, 64 x 8)
WRITER_SHAPES = [("auto", 128), ("auto", 512), (1, 4, 0), (4, 2, 2), (16, 8, 3), (64, 8, 3)]


def _wid(g):
    return f"auto-P{g[1]}" if g[0] == "auto" else _gid(g)


@pytest.fixture(scope="module", params=WRITER_SHAPES, ids=_wid)
def writer_eng(request):
    g = request.param
    for eng in engine_with(None if g[0] == "auto" else dict(zip(_KEYS, g))):
        eng.shape, eng.window_P = (None if g[0] == "auto" else g), (g[1] if g[0] == "auto" else lattice.geometry_P(g))
        eng.tag = _wid(g)
        yield eng


def _writer_lengths(eng, extra):
    return lattice.pass_lengths(eng.window_P, extra=extra, ks=(1,))


def test_patch_packed(writer_eng, pk):
    g = writer_eng.shape
    _packed_ipv4(writer_eng, pk, _writer_lengths(writer_eng, 60), 2, writer_eng.tag,
                 (lambda e, t: _ran(e, "ipv4", g[0], g[1], t)) if g else (lambda e, t: None))


def test_wrap_in_place_packed(writer_eng, pk):
    g = writer_eng.shape
    _packed_wrap(writer_eng, pk, _writer_lengths(writer_eng, 40), writer_eng.tag,
                 (lambda e, t: _ran(e, "wrap", g[0], g[1], t)) if g else (lambda e, t: None))


@pytest.mark.parametrize("apart", [False, True], ids=["in_place", "headers_apart"])
def test_router_packed(writer_eng, pk, apart):
    _packed_router(writer_eng, pk, _writer_lengths(writer_eng, 0), writer_eng.tag, apart)


# ------------------------------------------------------------ two-class ---
@pytest.fixture(scope="module", params=[{"twoclass": 8}, {"twoclass": 16}, {"twoclass": 32}], ids=force_id)
def two_eng(request):
    yield from engine_with(request.param)


def test_twoclass_checksum_packed(two_eng, pk):
    spw = two_eng.forced["twoclass"]
    _packed_checksum(two_eng, pk, lattice.twoclass_lengths(), f"twoclass {spw}", lambda e, t: _ran(e, "twoclass", 16, spw, t))


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["compute", "verify", "patch"])
def test_twoclass_ipv4_packed(two_eng, pk, mode):
    spw = two_eng.forced["twoclass"]
    _packed_ipv4(two_eng, pk, lattice.twoclass_lengths(60), mode, f"twoclass {spw}",
                 lambda e, t: _ran(e, "ipv4_twoclass", 16, spw, t))


# --------------------------------------------------------------- binned ---
@pytest.fixture(scope="module", params=[{"bin": 1, "bin_plan": 1}, {"bin": 1}], ids=force_id)
def bin_eng(request):
    yield from engine_with(request.param)


def test_binned_checksum_packed(bin_eng, pk):
    """E - 17 .. E + 17 around each bin edge: a segment binned by its length
    whose head sits late in its line can need a second pass in its bin's shape"""
    lengths = sorted({L for E in (144, 896, 1920, 4096) for L in range(E - 17, E + 18)})
    _packed_checksum(bin_eng, pk, lengths, force_id(bin_eng.forced), lambda e, t: _ran(e, "binned", tag=t))


# ================================================================ span =====
class _Span:
    """The window-edge lattice: one device row per batch (each row 256-byte
    aligned, so residues are the lattice's), version 4 and IHL 5..15 in turn
    at the target starts; references by (op, batch), shared by the engines."""

    def __init__(self, orc, seed):
        import torch

        rng = np.random.default_rng(seed)
        self.orc = orc
        self.batches = lattice.span_batches()
        self.n = self.batches[0][1].size - 1
        assert all(off.size - 1 == self.n for _, off in self.batches)
        self.row = (max(int(off[-1]) for _, off in self.batches) + 16 + 255) // 256 * 256
        self.buf = rng.integers(1, 256, (len(self.batches), self.row), dtype=np.uint8)
        for b, (lens, off) in enumerate(self.batches):
            s = off[1:-1:2].astype(np.int64)[lens[1::2] > 0]
            self.buf[b, s] = 0x40 | (5 + np.arange(s.size) % 11)
        self.init = rng.integers(0, 2**32, self.n, dtype=np.uint64).astype(np.uint32)
        self.odd = rng.integers(0, 2, self.n).astype(np.uint8)
        self.msgs = _msgs(rng, self.n)
        self.d0 = _t(self.buf)
        self.d = torch.empty_like(self.d0)
        self.d.copy_(self.d0)
        assert self.d.data_ptr() % 256 == 0 and self.d0.data_ptr() % 256 == 0
        self.doff = [_t(off) for _, off in self.batches]
        self.dinit, self.dodd = _t(self.init), _t(self.odd)
        self.dmsgs = _t(self.msgs.view(np.uint8).copy())
        self.ref = {}

    def want(self, op, b):
        key = (op, b)
        if key in self.ref:
            return self.ref[key]
        o, off, n = self.orc, self.batches[b][1], self.n
        hb = self.buf[b].copy()
        if op == "csum":
            r = o.checksum_batch(hb, n, offsets=off, init=self.init)
        elif op == "sum":
            r = o.sum_batch(hb, n, offsets=off, init=self.init, odd=self.odd)
        elif op.startswith("ipv4"):
            r = o.ipv4_tcp_batch(hb, n, int(op[-1]), offsets=off) + (hb,)
        else:
            s, ln = off[:-1].astype(np.int64), np.diff(off.astype(np.int64))
            apart = op == "apart"
            ok = np.ones(n, dtype=bool) if apart else ln >= 40
            hdr = _wrap_fields(self.msgs, ln + 40 if apart else ln)
            ip, tcp, st = ctypes.c_uint16(), ctypes.c_uint16(), ctypes.c_uint8()
            f = o.lib().orc_ipv4_tcp
            for i in np.flatnonzero(ok):
                if apart:
                    w = np.concatenate([hdr[i], hb[s[i]:s[i] + ln[i]]])
                    f(w.ctypes.data, w.size, 2, ctypes.byref(ip), ctypes.byref(tcp), ctypes.byref(st))
                    hdr[i] = w[:40]
                else:
                    hb[s[i]:s[i] + 40] = hdr[i]
                    f(hb.ctypes.data + int(s[i]), int(ln[i]), 2, ctypes.byref(ip), ctypes.byref(tcp), ctypes.byref(st))
                assert st.value & 3 == 3
            r = hdr if apart else hb
        self.ref[key] = r
        return r


@pytest.fixture(scope="module")
def sp(orc):
    return _Span(orc, 0x5BA2)


SPAN_FORCE = [{"tile": 1, "span_segs": 1}, {"tile": 1, "span_segs": 7}, {"tile": 1, "span_segs": 63},
              {"tile": 1, "span_segs": 7, "span_blocks": 5}]


@pytest.fixture(scope="module", params=SPAN_FORCE, ids=force_id)
def span_eng(request):
    yield from engine_with(request.param)


def _span_ran(eng, tag):
    _ran(eng, "tile", tag=tag)
    assert eng.dispatch_info()["lps"] == eng.forced["span_segs"], tag


def _span_where(sp, b, i):
    lens, off = sp.batches[b]
    return f"batch {b} (target length {int(lens[1])}), segment {i}, start residue {int(off[i]) % 128}"


def _span_cmp(sp, tag, what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    if bad.size:
        b, i = (int(v) for v in bad[0])
        pytest.fail(f"{tag} {what}: {_span_where(sp, b, i)}: got {int(got[b, i]):#x}, want {int(want[b, i]):#x}")


def test_span_checksum(span_eng, sp):
    import torch

    tag, B = force_id(span_eng.forced), len(sp.batches)
    o16, o32 = _rows(B, sp.n, torch.int16), _rows(B, sp.n, torch.int32)
    for b in range(B):
        span_eng.checksum_batch(sp.d0[b], offsets=sp.doff[b], init=sp.dinit, out=o16[b])
        _span_ran(span_eng, (tag, b))
        span_eng.sum_batch(sp.d0[b], offsets=sp.doff[b], init=sp.dinit, odd=sp.dodd, out=o32[b])
        _span_ran(span_eng, (tag, b))
    _span_cmp(sp, tag, "checksum", _u16(o16), [sp.want("csum", b) for b in range(B)])
    _span_cmp(sp, tag, "sum", _u32(o32), [sp.want("sum", b) for b in range(B)])


def _span_bytes(sp, tag, what, got, want_of):
    for b in range(len(sp.batches)):
        bad = np.flatnonzero(got[b] != want_of(b))
        if bad.size:
            off = sp.batches[b][1]
            i = int(np.searchsorted(off, int(bad[0]), side="right")) - 1
            pytest.fail(f"{tag} {what}: byte {int(bad[0])}, {_span_where(sp, b, min(max(i, 0), sp.n - 1))}")


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["compute", "verify", "patch"])
def test_span_ipv4(span_eng, sp, mode):
    import torch

    tag, B = force_id(span_eng.forced), len(sp.batches)
    ip, tcp, st = _rows(B, sp.n, torch.int16), _rows(B, sp.n, torch.int16), _rows(B, sp.n, torch.uint8)
    sp.d.copy_(sp.d0)
    for b in range(B):
        span_eng.ipv4_tcp_batch(sp.d[b], mode, offsets=sp.doff[b], ip_ck=ip[b], tcp_ck=tcp[b], status=st[b])
        _span_ran(span_eng, (tag, b))
    want = [sp.want(f"ipv4_{mode}", b) for b in range(B)]
    _span_cmp(sp, tag, f"mode {mode} ip_ck", _u16(ip), [w[0] for w in want])
    _span_cmp(sp, tag, f"mode {mode} tcp_ck", _u16(tcp), [w[1] for w in want])
    _span_cmp(sp, tag, f"mode {mode} status", st.cpu().numpy(), [w[2] for w in want])
    _span_bytes(sp, tag, f"mode {mode} bytes", sp.d.cpu().numpy(), lambda b: want[b][3])
    sp.d.copy_(sp.d0)


def test_span_wrap_in_place(span_eng, sp):
    tag = force_id(span_eng.forced)
    sp.d.copy_(sp.d0)
    for b in range(len(sp.batches)):
        span_eng.tcp_wrap_batch(sp.d[b], sp.dmsgs, n=sp.n, offsets=sp.doff[b])
        _span_ran(span_eng, (tag, b))
    _span_bytes(sp, tag, "wrap bytes", sp.d.cpu().numpy(), lambda b: sp.want("wrap", b))
    sp.d.copy_(sp.d0)


def test_span_wrap_headers_apart(span_eng, sp):
    import torch

    tag, B = force_id(span_eng.forced), len(sp.batches)
    hd = torch.full((B, sp.n * 40), 0xA5, dtype=torch.uint8, device="cuda:0")
    for b in range(B):
        span_eng.tcp_wrap_headers(sp.d0[b], sp.dmsgs, hd[b], n=sp.n, offsets=sp.doff[b])
        _span_ran(span_eng, (tag, b))
    got = hd.cpu().numpy().reshape(B, sp.n, 40)
    bad = np.argwhere((got != np.stack([sp.want("apart", b) for b in range(B)])).any(axis=2))
    if bad.size:
        b, i = (int(v) for v in bad[0])
        pytest.fail(f"{tag} header: {_span_where(sp, b, i)}")
    assert (sp.d0.cpu().numpy() == sp.buf).all(), (tag, "the payloads changed")
