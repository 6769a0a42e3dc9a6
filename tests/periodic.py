"""Periodic batches for the route, frame and unwrap families: K = 4099 distinct
items built on the CPU with the suites' own generators (test_gpu_frames'
make_burst, test_gpu_unwrap's length / header / data-offset mix, the frame
tests' destination pool), their expectations from the restatements
(route_ref.py, frame_ref.py, unwrap_ref.py), and the device-side tiling that
turns both into a batch of any n without another byte crossing the bus.  K is
prime, so the period never lines up with a wave (64 lanes), a block (256) or the
grid.  Shared by test_gpu_grid_stride.py and test_gpu_concurrency_tables.py;
test_periodic_inputs (test_shape_lattice_headers.py) checks on the CPU that
every status class is present."""
import random

import numpy as np

from frame_ref import forward_header, ipv4_parses
from route_ref import NO_ROUTE, boundary_addrs
from unwrap_ref import make_dgram, unwrap

K = 4099
FRAME_STRIDE, FRAME_LEN = 64, 60
UNWRAP_LENGTHS = [0, 19, 20, 39, 40, 41, 59, 60, 61, 64]  # test_gpu_unwrap's LENGTHS; 1500 once in 64 (below)
HLENS, DOFFS = [5, 6, 15], [4, 5, 6, 15]


def frame_items(seed=0x9E1D):
    """(frames, ins): K frames of 60 bytes with test_gpu_frames' mix of classes"""
    from test_gpu_frames import make_burst

    return make_burst(seed, [FRAME_LEN] * K)


def frames_fixed(frames):
    """the frames at stride 64, 0xA5 in the four bytes between them"""
    buf = np.full((len(frames), FRAME_STRIDE), 0xA5, np.uint8)
    buf[:, :FRAME_LEN] = np.frombuffer(b"".join(frames), np.uint8).reshape(len(frames), FRAME_LEN)
    return buf.reshape(-1)


def dgram_items(seed=0xD61A):
    """the router calls' datagrams: frames of test_gpu_frames' length mix behind
    their Ethernet header (0..46 bytes, one in a hundred 1500), each at its own length"""
    from test_gpu_frames import MIX, make_burst

    lengths = np.random.default_rng(seed).choice(MIX, K, p=[.03, .03, .04, .05, .25, .05, .24, .30, .01])
    return [f[14:] for f in make_burst(seed, lengths)[0]]


def unwrap_items(seed=0x0B5E):
    rng = random.Random(seed)
    out = []
    for i in range(K):
        n = 1500 if i % 64 == 63 else rng.choice(UNWRAP_LENGTHS) if rng.random() < 0.7 else rng.randrange(0, 130)
        out.append(make_dgram(rng, n, rng.choice(HLENS + [4]), rng.choice(DOFFS)))
    return out


def addr_items(routes, seed=0xADD2):
    """K host-order addresses: every route's boundary addresses, addresses under
    a route's prefix with random low bits (half of the rest), random ones"""
    rng = np.random.default_rng(seed)
    edge = np.array(boundary_addrs(routes), np.uint32)[:K // 3]
    rest = rng.integers(0, 2**32, K - edge.size, dtype=np.uint64)
    under = np.array([r[0] for r in routes], np.uint64)[rng.integers(0, len(routes), rest.size)]
    low = rest & ((np.uint64(1) << rng.integers(0, 25, rest.size).astype(np.uint64)) - np.uint64(1))
    rest = np.where(rng.random(rest.size) < 0.5, under | low, rest)
    return np.concatenate([edge, rest.astype(np.uint32)])[rng.permutation(K)]


def pack(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items), np.uint8).copy(), off


def route_expect(dgrams, router):
    """Router::route over raw datagrams: (status n, iface n, next_hop n,
    headers n x 20, the datagrams as the in-place call leaves them)"""
    n = len(dgrams)
    st, fi, fh = np.zeros(n, np.uint8), np.full(n, NO_ROUTE, np.uint32), np.zeros(n, np.uint32)
    hd, after = np.zeros((n, 20), np.uint8), []
    for i, p in enumerate(dgrams):
        hdr = forward_header(p) if ipv4_parses(p) else None
        if hdr is not None:
            st[i] = 1
            hd[i] = np.frombuffer(hdr, np.uint8)
            hit = router.answer(int.from_bytes(p[16:20], "big"))
            if hit is not None:
                st[i], fi[i], fh[i] = 3, hit[0], hit[1]
        after.append(p if hdr is None else hdr + p[20:])
    return st, fi, fh, hd, after


def unwrap_expect(dgrams):
    return np.frombuffer(b"".join(unwrap(d) for d in dgrams), np.uint8).reshape(len(dgrams), 40)


# ------------------------------------------------------------ on the device --
def tile(t, n, width=1):
    """the K-item device tensor `t` (K x width elements, flat) repeated to n items"""
    reps = -(-n // K)
    return t.repeat(reps)[:n * width]


def tile_offsets(off, n):
    """K + 1 packed offsets repeated to n + 1: block r starts where block r - 1 ended"""
    import torch

    o = torch.from_numpy(off.astype(np.int64)).cuda()
    reps = -(-n // K)
    starts = (o[:K].repeat(reps).view(reps, K) + (torch.arange(reps, device=o.device) * int(off[-1])).view(reps, 1))
    out = torch.empty(n + 1, dtype=torch.int64, device=o.device)
    out[:n] = starts.view(-1)[:n]
    out[n] = out[n - 1] + int(off[(n - 1) % K + 1] - off[(n - 1) % K])
    return out


def sentinel(n, dtype, value, tail=64):
    """(the whole tensor, its first n elements): `tail` sentinel elements behind the output"""
    import torch

    whole = torch.full((n + tail,), value, dtype=dtype, device="cuda:0")
    return whole, whole[:n]


def tail_untouched(whole, n, value):
    return bool((whole[n:] == value).all())


# ------------------------------------------------------- classes, asserted --
def assert_frame_classes(st):
    """every status bit of the hop, every strict step of the implication chain, and nothing at all"""
    from frame_ref import FR_ARP, FR_ARP_OK, FR_DGRAM, FR_FOR_US, FR_IPV4, FR_RESOLVED, RT_FORWARD, RT_ROUTED

    st = np.asarray(st)
    for bit in (FR_RESOLVED, RT_ROUTED, RT_FORWARD, FR_DGRAM, FR_IPV4, FR_FOR_US, FR_ARP, FR_ARP_OK):
        assert (st & bit != 0).any(), bit
    for a, b in ((RT_ROUTED, FR_RESOLVED), (RT_FORWARD, RT_ROUTED), (FR_DGRAM, RT_FORWARD), (FR_IPV4, FR_DGRAM),
                 (FR_FOR_US, FR_IPV4 | FR_ARP), (FR_ARP, FR_ARP_OK)):
        assert ((st & a != 0) & (st & b == 0)).any(), (a, b)
    assert (st == 0).any()


def assert_route_classes(st, matched=None):
    """dropped, forwarded without a route, forwarded and routed; a lookup batch: hits and misses"""
    assert set(np.unique(st)) == {0, 1, 3}
    if matched is not None:
        assert 0 < int(np.sum(matched)) < len(matched)


def assert_unwrap_classes(rec, dgrams):
    """test_gpu_unwrap's classes: nothing, accepted, parsed but not TCP, a header
    that does not parse, no TCP header, a bad TCP checksum, both header-load paths"""
    st = rec[:, 36]
    hlen = np.array([d[0] & 15 if d else 0 for d in dgrams])
    assert (st == 0).any() and (st == 0x0F).any() and (st == 0x07).any()
    assert ((st & 1 == 0) & (st != 0)).any()
    assert ((st & 3 == 3) & (st & 4 == 0)).any()
    assert ((st & 5 == 5) & (st & 2 == 0)).any()
    assert ((st & 7 == 7) & (hlen > 5)).any() and ((st & 7 == 7) & (hlen == 5)).any()
    assert (rec[(st & 7) != 7][:, :36] == 0).all()


# ------------------------------------------------------- batch-size sweep --
# every n of two waves and a bit (an idle lane group, a partial last wave of 1..63, the second wave's first
# lanes), the 255 / 256 / 257 block edge and the second block's
SWEEP_NS = list(range(131)) + [255, 256, 257, 511, 512, 513]
SWEEP_MAX = max(SWEEP_NS)


def sweep_sizes(call, specs, wants):
    """One call per n of SWEEP_NS on the first n items of one uploaded batch of SWEEP_MAX items.
    `call(n, outs)` makes the call into `outs` (views of n items); `specs`: (dtype, elements per item, sentinel)
    per output; `wants`: the SWEEP_MAX-item expectations (numpy).  Every output is sentinel-filled before each
    call and compared in full behind it: the first n items, and everything after them untouched — n = 0 writes
    nothing."""
    import torch

    from test_gpu_parity import _t

    wholes = [torch.empty(SWEEP_MAX * w + 64, dtype=dt, device="cuda:0") for dt, w, _ in specs]
    wants = [_t(np.ascontiguousarray(x).reshape(-1)) for x in wants]
    for n in SWEEP_NS:
        for whole, (_, _, v) in zip(wholes, specs):
            whole.fill_(v)
        call(n, [whole[:n * w] for whole, (_, w, _) in zip(wholes, specs)])
        for k, (whole, want, (_, w, v)) in enumerate(zip(wholes, wants, specs)):
            assert torch.equal(whole[:n * w], want[:n * w]), (n, k, (whole[:n * w] != want[:n * w]).nonzero()[:4].tolist())
            assert bool((whole[n * w:] == v).all()), (n, k, "written behind the output")
