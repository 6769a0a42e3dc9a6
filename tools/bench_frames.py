#!/usr/bin/env python3
"""Dev measurement: what the Ethernet layer costs on top of the router batch.

Shape: 1 M x 1514 B frames (ttl = i % 4, half dropped), addressed to the ingress
interface, the IPv4 datagram 14 bytes in; the same datagrams once more at
stride 1500 for the calls that take bare datagrams.  1000 routes of /8../16
over 8 interfaces, every other one with a next hop; 9 in 10 destinations under
a route.  Per neighbour table — about 1000 and about 50 000 mappings (the
gateways first, then the destinations of directly routed datagrams) — the rows

  route_headers   ics_router_route_headers, datagrams at stride 1500 (the merged hop)
  router_frames   ics_router_frames, frames at stride 1514
  ttl_headers     ics_router_ttl_headers, datagrams at stride 1500 (the bare step)
  frame_recv      ics_frame_recv_batch, frames at stride 1514

each timed with device events around one call after a synchronise, the
variants alternating inside every round, median of ROUNDS (>= 50) rounds after
5 warm-up rounds.  Before timing, router_frames' status & 3, record[16:36],
interfaces and next hops are compared with route_headers'.  Then one host
row: tools/probe/resolve_loop, the per-datagram ics_neigh_table_resolve loop
the fused call replaces, on 16 threads (built on first use).
One JSON line per row on stdout (and appended to the file given as argv[1])."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_route import dsts_for, table_short, timed  # noqa: E402
from tcpip_network_protocol_stack_amd.engine import Engine, NeighTable, RouteTable  # noqa: E402

N, L, F, SEED = 1 << 20, 1500, 1514, 0x7008
ROUNDS = int(os.environ.get("FRAME_ROUNDS", "60"))
IFACES = 8


def host_row(mappings):
    exe = os.path.join(ROOT, "tools", "probe", "resolve_loop")
    if not os.path.exists(exe):
        csrc = os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                               exe + ".cpp", os.path.join(csrc, "icsum_neigh.cpp"), "-o", exe, "-lpthread"])
    return json.loads(subprocess.check_output([exe, str(mappings), str(N), "16"], text=True))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    eng = Engine(0)
    rng = np.random.default_rng(SEED)
    d = eng.fill_bytes(torch.empty(N * L, dtype=torch.uint8, device="cuda:0"), SEED)
    eng.ipv4_tcp_headers(d, N, L, L, SEED)
    v = d.view(N, L)
    v[:, 8] = (torch.arange(N, device=d.device) % 4).to(torch.uint8)
    routes = table_short(rng)
    tbl = RouteTable()
    hops = {}
    for k, (p, ln) in enumerate(routes):
        nh = None if k % 2 else 0x0A000001 + k
        tbl.add(p, ln, k % IFACES, nh)
    dst = dsts_for(rng, routes)
    v[:, 16:20] = torch.from_numpy(dst.byteswap().view(np.uint8).reshape(N, 4).copy()).cuda()
    eng.ipv4_tcp_batch(d, 2, n=N, stride=L, dgram_len=L)  # both checksums for the new ttl and dst
    macs = [bytes([2, 0, 0, 0, 0, k]) for k in range(IFACES)]
    fr = torch.empty(N * F, dtype=torch.uint8, device="cuda:0")
    fv = fr.view(N, F)
    fv[:, 14:] = v
    fv[:, :14] = torch.tensor(list(macs[0] + bytes([2, 0, 0, 0, 0, 0x55]) + b"\x08\x00"), dtype=torch.uint8,
                              device="cuda:0")
    hd0 = torch.empty(N * 20, dtype=torch.uint8, device="cuda:0")
    hd2 = torch.empty_like(hd0)
    hd1 = torch.empty(N * 36, dtype=torch.uint8, device="cuda:0")
    st0, st1, st2, st3 = (torch.empty(N, dtype=torch.uint8, device="cuda:0") for _ in range(4))
    f0, h0, f1, h1 = (torch.empty(N, dtype=torch.int32, device="cuda:0") for _ in range(4))
    # what each datagram's hop is, from the merged call
    eng.router_route_headers(tbl, d, n=N, stride=L, dgram_len=L, hdrs=hd0, status=st0, iface=f0, next_hop=h0)
    torch.cuda.synchronize()
    routed = (st0.cpu().numpy() & 2) != 0
    pairs = np.stack([f0.cpu().numpy().view(np.uint32)[routed], h0.cpu().numpy().view(np.uint32)[routed]], axis=1)
    uniq, counts = np.unique(pairs, axis=0, return_counts=True)
    order = np.argsort(-counts, kind="stable")  # the gateways (many datagrams each) first
    rows = []
    for target in (1000, 50_000):
        nt = NeighTable()
        for k in range(IFACES):
            nt.set_iface(k, macs[k], 0x0A000001 + (k << 8))
        for k in order[:target]:
            nt.learn(int(uniq[k, 0]), int(uniq[k, 1]), bytes([6, 0]) + int(k).to_bytes(4, "big"))
        stats = nt.stats()
        variants = {
            "route_headers": lambda: eng.router_route_headers(tbl, d, n=N, stride=L, dgram_len=L, hdrs=hd0, status=st0,
                                                              iface=f0, next_hop=h0),
            "router_frames": lambda: eng.router_frames(tbl, nt, fr, n=N, stride=F, frame_len=F, hdrs=hd1, status=st1,
                                                       iface=f1, next_hop=h1),
            "ttl_headers": lambda: eng.router_ttl_headers(d, n=N, stride=L, dgram_len=L, hdrs=hd2, status=st2),
            "frame_recv": lambda: eng.frame_recv(nt, fr, n=N, stride=F, frame_len=F, status=st3),
        }
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(st1 & 3, st0) and torch.equal(hd1.view(N, 36)[:, 16:], hd0.view(N, 20))
        assert torch.equal(f1, f0) and torch.equal(h1, h0)
        assert bool(((st1 & 0x30) == 0x30).all()) and torch.equal(st3, st1 & 0xF8)
        resolved = int(((st1 & 4) != 0).sum())
        ts = {k: [] for k in variants}
        for r in range(ROUNDS + 5):
            for k, fn in variants.items():
                t = timed(fn)
                if r >= 5:
                    ts[k].append(t)
        for k, xs in ts.items():
            xs.sort()
            row = {"neigh": stats["mappings"], "row": k, "n": N, "frame_len": F,
                   "median_us": round(statistics.median(xs), 2), "p10_us": round(xs[len(xs) // 10], 2),
                   "p90_us": round(xs[(9 * len(xs)) // 10], 2), "rounds": len(xs),
                   "image_bytes": 16 * (stats["image_ifaces"] + stats["image_slots"]),
                   "forwarded": int((st0 & 1).sum()), "routed": int(routed.sum()), "resolved": resolved}
            rows.append(row)
            print(json.dumps(row), flush=True)
        row = host_row(stats["mappings"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        nt.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
