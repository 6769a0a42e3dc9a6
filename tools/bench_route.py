#!/usr/bin/env python3
"""Dev measurement: what the route lookup costs on top of the bare router step.

Shape: config "7" at 1 M x 1500 B datagrams (ttl = i % 4, half dropped),
headers apart.  Per table — (a) 1000 routes of /8../16 (a 256 KiB image),
(b) 50 000 routes, mostly /8../24 with some /25../31, (c) 80 000 /17 routes,
two under each of 40 000 distinct /16s (an image of about 42 MB whose every
level-2 word is an answer: far past an XCD's 4 MiB L2) — every datagram's dst is drawn from the
table's routes (9 in 10) or at random (1 in 10), and the rows are

  bare           ics_router_ttl_headers
  fused          ics_router_route_headers
  bare+lookup    ics_router_ttl_headers, then ics_route_lookup_batch on the dsts
  lookup         ics_route_lookup_batch alone, 1 M addresses

each timed with device events around one call after a synchronise, the
variants alternating inside every round, median of ROUNDS (>= 50) rounds after
5 warm-up rounds.  Before timing, the fused call's headers and forward bits
are compared with the bare call's and its answers with the lookup batch's.
One JSON line per row on stdout (and appended to the file given as argv[1])."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tcpip_network_protocol_stack_amd.engine import Engine, RouteTable  # noqa: E402

N, L, SEED = 1 << 20, 1500, 0x7007
ROUNDS = int(os.environ.get("ROUTE_ROUNDS", "60"))


def mask_of(length):
    return (0xFFFFFFFF << (32 - length)) & 0xFFFFFFFF


def table_short(rng):
    lens = rng.integers(8, 17, 1000)
    return [(int(rng.integers(0, 2**32)) & mask_of(int(k)), int(k)) for k in lens]


def table_50k(rng):
    lens = rng.choice(list(range(8, 25)) * 6 + list(range(25, 32)), 50_000)
    return [(int(rng.integers(0, 2**32)) & mask_of(int(k)), int(k)) for k in lens]


def table_large(rng):
    hi = rng.permutation(1 << 16)[:40_000]
    return [((int(h) << 16) | half, 17) for h in hi for half in (0, 0x8000)]


def dsts_for(rng, routes):
    """9 in 10 under a route drawn uniformly (random host bits), the rest random"""
    r = rng.integers(0, len(routes), N)
    pre = np.array([p for p, _ in routes], dtype=np.uint64)[r]
    ln = np.array([k for _, k in routes], dtype=np.uint64)[r]
    host = rng.integers(0, 2**32, N, dtype=np.uint64) & ((np.uint64(1) << (np.uint64(32) - ln)) - np.uint64(1))
    d = pre | host
    rnd = rng.random(N) < 0.1
    d[rnd] = rng.integers(0, 2**32, int(rnd.sum()), dtype=np.uint64)
    return d.astype(np.uint32)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3  # us


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    eng = Engine(0)
    rng = np.random.default_rng(SEED)
    d = eng.fill_bytes(torch.empty(N * L, dtype=torch.uint8, device="cuda:0"), SEED)
    eng.ipv4_tcp_headers(d, N, L, L, SEED)
    v = d.view(N, L)
    v[:, 8] = (torch.arange(N, device=d.device) % 4).to(torch.uint8)
    hd0 = torch.empty(N * 20, dtype=torch.uint8, device="cuda:0")
    hd1 = torch.empty_like(hd0)
    st0 = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    st1 = torch.empty_like(st0)
    f1 = torch.empty(N, dtype=torch.int32, device="cuda:0")
    h1 = torch.empty_like(f1)
    f2, h2 = torch.empty_like(f1), torch.empty_like(f1)
    rows = []
    for name, make in (("le16_1000", table_short), ("mixed_50000", table_50k), ("slash17_80000_large", table_large)):
        routes = make(rng)
        tbl = RouteTable()
        for k, (p, ln) in enumerate(routes):
            tbl.add(p, ln, k % 64, None if k % 2 else 0x0A000001 + k)
        stats = tbl.stats()
        dst = dsts_for(rng, routes)
        be = torch.from_numpy(dst.byteswap().view(np.uint8).reshape(N, 4).copy()).cuda()
        v[:, 16:20] = be
        eng.ipv4_tcp_batch(d, 2, n=N, stride=L, dgram_len=L)  # both checksums for the new ttl and dst
        addrs = torch.from_numpy(dst.view(np.int32).copy()).cuda()
        variants = {
            "bare": lambda: eng.router_ttl_headers(d, n=N, stride=L, dgram_len=L, hdrs=hd0, status=st0),
            "fused": lambda: eng.router_route_headers(tbl, d, n=N, stride=L, dgram_len=L, hdrs=hd1, status=st1,
                                                      iface=f1, next_hop=h1),
            "bare+lookup": lambda: (eng.router_ttl_headers(d, n=N, stride=L, dgram_len=L, hdrs=hd0, status=st0),
                                    eng.route_lookup_batch(tbl, addrs, iface=f2, next_hop=h2)),
            "lookup": lambda: eng.route_lookup_batch(tbl, addrs, iface=f2, next_hop=h2),
        }
        # same results first: the fused call against the bare step and the lookup batch
        variants["bare+lookup"]()
        variants["fused"]()
        torch.cuda.synchronize()
        fwd = st0 == 1
        assert torch.equal(hd0, hd1) and torch.equal(st1 & 1, st0)
        routed = (st1 & 2) != 0
        assert torch.equal(routed, fwd & (f2 != -1))
        assert torch.equal(f1[routed], f2[routed]) and torch.equal(h1[routed], h2[routed])
        assert bool((f1[~routed] == -1).all()) and bool((h1[~routed] == 0).all())
        ts = {k: [] for k in variants}
        for r in range(ROUNDS + 5):
            for k, fn in variants.items():
                t = timed(fn)
                if r >= 5:
                    ts[k].append(t)
        for k, xs in ts.items():
            xs.sort()
            row = {"table": name, "row": k, "n": N, "dgram_len": L, "median_us": round(statistics.median(xs), 2),
                   "p10_us": round(xs[len(xs) // 10], 2), "p90_us": round(xs[(9 * len(xs)) // 10], 2),
                   "rounds": len(xs), "image_bytes": 4 * (stats["image_words"] + 2 * stats["route_records"]),
                   "l2_chunks": stats["l2_chunks"], "l3_chunks": stats["l3_chunks"],
                   "forwarded": int(fwd.sum()), "routed": int(routed.sum())}
            rows.append(row)
            print(json.dumps(row), flush=True)
        tbl.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
