#!/usr/bin/env python3
"""Dev measurement: what the message records cost on top of the VERIFY pass.

Shapes (valid IPv4 / TCP headers, both checksums set by a PATCH pass):

  mtu_1m     1 M x 1500 B, fixed stride
  mix_1m     1 M datagrams, half 40 B ACKs / half 1500 B, packed offsets
  tick_256k  the stack tick's receive batch: 256 Ki of the same mix

Per shape the rows

  verify     ics_ipv4_tcp_batch ICS_MODE_VERIFY, status only (code the parent
             commit already has: the yardstick)
  unwrap     ics_tcp_unwrap_batch with d_status (the same VERIFY dispatch, then
             k_tcp_unwrap)
  records    unwrap - verify, paired per round: the cost of the records launch

each call timed with device events around one call after a synchronise, the
two alternating inside every round, median of ROUNDS (>= 50) rounds after 5
warm-up rounds, in one process on one box.  Before timing, the records' status
bytes are compared with VERIFY's and every record with
ics_tcp_unwrap_one's on a sample.  `traffic_mb` is what the records launch has
to move at least (two 64-byte lines in and 41 bytes out per datagram) and
`floor_us` that over 8 TB/s.  Then one host row per shape:
tools/probe/unwrap_loop, ics_tcp_unwrap_one per datagram on 1 and on 16 threads
(built on first use).  One JSON line per row on stdout (and appended to the
file given as argv[1])."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_route import timed  # noqa: E402
from tcpip_network_protocol_stack_amd.engine import Engine, tcp_unwrap_one  # noqa: E402

ROUNDS = int(os.environ.get("UNWRAP_ROUNDS", "60"))
SEED = 0x756E
SHAPES = (("mtu_1m", 1 << 20, False), ("mix_1m", 1 << 20, True), ("tick_256k", 1 << 18, True))


def host_rows(shape, n):
    exe = os.path.join(ROOT, "tools", "probe", "unwrap_loop")
    if not os.path.exists(exe):
        csrc = os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), exe + ".cpp",
                               os.path.join(csrc, "icsum_unwrap.cpp"), "-o", exe, "-lpthread"])
    return [json.loads(subprocess.check_output([exe, "mix" if shape != "mtu_1m" else "mtu", str(n), str(t)], text=True))
            for t in (1, 16)]


def make(eng, n, mix):
    """(datagram tensor, offsets tensor or None, addressing kwargs, host lengths)"""
    dev = "cuda:0"
    if not mix:
        L = 1500
        d = eng.fill_bytes(torch.empty(n * L, dtype=torch.uint8, device=dev), SEED)
        eng.ipv4_tcp_headers(d, n, L, L, SEED)
        kw = {"stride": L, "dgram_len": L}
        eng.ipv4_tcp_batch(d, 2, n=n, **kw)
        return d, None, kw, np.full(n, L)
    rng = np.random.default_rng(SEED + n)
    rl = np.where(rng.random(n) < 0.5, 40, 1500)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(rl)
    buf = rng.integers(0, 256, int(off[-1]) + 16, dtype=np.uint8)
    rs = off[:-1].astype(np.int64)
    buf[rs], buf[rs + 1], buf[rs + 2], buf[rs + 3] = 0x45, 0, (rl >> 8).astype(np.uint8), (rl & 255).astype(np.uint8)
    buf[rs + 6], buf[rs + 7], buf[rs + 8], buf[rs + 9], buf[rs + 32] = 0x40, 0, 64, 6, 0x50
    d = torch.from_numpy(buf).to(dev)
    doff = torch.from_numpy(off.view(np.int64)).to(dev)
    kw = {"offsets": doff}
    eng.ipv4_tcp_batch(d, 2, n=n, **kw)
    return d, off, kw, rl


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    eng = Engine(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for shape, n, mix in SHAPES:
        d, off, kw, lens = make(eng, n, mix)
        st0 = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        st1 = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        recs = torch.empty(n * 40, dtype=torch.uint8, device="cuda:0")
        o = kw.get("offsets")
        args = (d.data_ptr(), o.data_ptr() if o is not None else None, kw.get("stride", 0), kw.get("dgram_len", 0), n)

        def verify():  # status only, as the unwrap's own VERIFY leg asks for it
            eng._check(eng.lib.ics_ipv4_tcp_batch(eng.ctx, *args, 1, None, None, st0.data_ptr(), stream))

        def unwrap():
            eng._check(eng.lib.ics_tcp_unwrap_batch(eng.ctx, *args, recs.data_ptr(), st1.data_ptr(), stream))

        kernels = {}
        for _ in range(3):  # the plan cache lands (offsets batches): steady-state dispatch for both
            verify()
            torch.cuda.synchronize()
            kernels["verify"] = eng.dispatch_info()
            unwrap()
            torch.cuda.synchronize()
        assert eng.dispatch_info()["kernel"] == "unwrap"
        r = recs.view(n, 40)
        assert torch.equal(st0, st1) and torch.equal(r[:, 36], st0)
        parsed = int(((st0 & 7) == 7).sum())
        assert parsed == n, (parsed, n)
        host = d.cpu().numpy()
        starts = off[:-1].astype(np.int64) if off is not None else np.arange(n, dtype=np.int64) * 1500
        rh = r.cpu().numpy()
        for i in np.random.default_rng(1).integers(0, n, 2000):
            w = host[starts[i]:starts[i] + lens[i]].tobytes()
            assert bytes(tcp_unwrap_one(w)) == rh[i].tobytes(), i
        ts = {"verify": [], "unwrap": [], "records": []}
        for rnd in range(ROUNDS + 5):
            order = (verify, unwrap) if rnd % 2 == 0 else (unwrap, verify)  # alternate who goes first
            t = {fn.__name__: timed(fn) for fn in order}
            if rnd >= 5:
                ts["verify"].append(t["verify"])
                ts["unwrap"].append(t["unwrap"])
                ts["records"].append(t["unwrap"] - t["verify"])
        nbytes = int(lens.sum())
        traffic = n * (2 * 64 + 41)
        for k, xs in ts.items():
            xs.sort()
            row = {"shape": shape, "row": k, "n": n, "bytes": nbytes, "median_us": round(statistics.median(xs), 2),
                   "p10_us": round(xs[len(xs) // 10], 2), "p90_us": round(xs[(9 * len(xs)) // 10], 2),
                   "rounds": len(xs), "verify_kernel": kernels["verify"]["kernel"],
                   "verify_lps": kernels["verify"]["lps"], "parsed": parsed}
            if k == "records":
                row["traffic_mb"] = round(traffic / 1e6, 1)
                row["floor_us"] = round(traffic / 8e12 * 1e6, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        for row in host_rows(shape, n):
            rows.append(row)
            print(json.dumps(row), flush=True)
        del d, recs, st0, st1
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
