#!/usr/bin/env python3
"""Dev measurement: what the receive streams' copy costs (k_copy_pieces) and
what the host plan in front of it costs per record.

Shapes (payloads in order, one piece per data segment, each from its
datagram's byte 40 on into consecutive ring bytes):

  mtu_1m     1 M x 1460 B payloads out of 1500-byte datagrams, fixed stride
  tick_256k  the stack tick's receive mix: 256 Ki datagrams, half 40 B ACKs
             (no piece) / half 1500 B, packed offsets
  small_1m   1 M x 100 B payloads out of 140-byte datagrams, fixed stride

Per shape the rows

  copy    ics_copy_pieces over the shape's pieces, already in device memory
  memcpy  a device-to-device hipMemcpyAsync (torch copy_) of the same byte
          count in the same process: the neighbour measurement
  plan    ics_rx_stream_plan on the host over the shape's records (a fresh
          stream object per round, capacity 2^30; mtu_1m plans the 735 439
          records that fit that capacity) — per call and per record
  receive_batch  the feature's own call, ics_rx_stream_receive_batch, over the
          same records into a fresh stream's ring (RX_ROUNDS rounds): device
          events around the call, so the host plan, the list's copy into its
          page-locked slot, its DMA to the device (`list_mb`) and the copy
          kernel are all inside; `host_call_us` is the call's own return time
  host_path  tools/probe/reasm_loop: the host payload path the feature
          replaces (unwrap_records' payload copy plus the reference's
          per-segment string operations), 1 and 16 threads alternating

copy and memcpy are timed with device events around one call after a
synchronise, the two alternating inside every round, median of ROUNDS (>= 50)
rounds after 5 warm-up rounds, in one process on one box.  Before timing the
copy's result is compared with torch's own gather.  `traffic_mb` is what the
copy has to move (bytes read + bytes written + 16 B per piece) and `floor_us`
that over 8 TB/s.  One JSON line per row on stdout (and appended to the file
given as argv[1])."""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_route import timed  # noqa: E402
from tcpip_network_protocol_stack_amd.engine import COPY_PIECE_DTYPE, TCP_RX_DTYPE, Engine, RxStream  # noqa: E402

ROUNDS = int(os.environ.get("REASM_ROUNDS", "60"))
RX_ROUNDS = int(os.environ.get("REASM_RX_ROUNDS", "15"))
SEED = 0x7265
ISN = 1000


def shape(name):
    """(datagram lengths, payload lengths) of a shape; payloads start at byte 40"""
    if name == "mtu_1m":
        n = 1 << 20
        return np.full(n, 1500), np.full(n, 1460)
    if name == "small_1m":
        n = 1 << 20
        return np.full(n, 140), np.full(n, 100)
    n = 1 << 18
    rl = np.where(np.random.default_rng(SEED).random(n) < 0.5, 40, 1500)
    return rl, rl - 40


def host_rows(name, n):
    exe = os.path.join(ROOT, "tools", "probe", "reasm_loop")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", exe + ".cpp", "-o", exe, "-lpthread"])
    kind = {"mtu_1m": "mtu", "small_1m": "small", "tick_256k": "tick"}[name]
    out = subprocess.check_output([exe, kind, str(n), "1,16", "9"], text=True)
    return [json.loads(line) for line in out.splitlines()]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    eng = Engine(0)
    rows = []
    for name in ("mtu_1m", "tick_256k", "small_1m"):
        dl, pl = shape(name)
        n = len(dl)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum(dl)
        idx = np.zeros(n + 1, dtype=np.uint64)
        idx[1:] = np.cumsum(pl)
        total = int(idx[-1])
        data = pl > 0
        pieces = np.zeros(int(data.sum()), COPY_PIECE_DTYPE)
        pieces["src"], pieces["dst"], pieces["len"] = off[:-1][data] + 40, idx[:-1][data], pl[data]
        m = len(pieces)
        # 40 bytes in front: the SYN's datagram of the receive_batch rows
        src_full = eng.fill_bytes(torch.empty(40 + int(off[-1]), dtype=torch.uint8, device="cuda:0"), SEED)
        src = src_full[40:]
        dst = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        plain = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        dp = torch.from_numpy(pieces.view(np.uint8)).cuda()

        def copy():
            eng.copy_pieces(src, dst, dp, m=m)

        def memcpy():
            plain.copy_(src[:total], non_blocking=True)

        copy()
        torch.cuda.synchronize()
        assert eng.dispatch_info()["kernel"] == "copy_pieces"
        for k in np.random.default_rng(1).integers(0, m, 4000):  # the copy against torch's own slices
            p = pieces[k]
            assert torch.equal(dst[int(p["dst"]):int(p["dst"]) + int(p["len"])],
                               src[int(p["src"]):int(p["src"]) + int(p["len"])]), k
        ts = {"copy": [], "memcpy": []}
        for rnd in range(ROUNDS + 5):
            order = (copy, memcpy) if rnd % 2 == 0 else (memcpy, copy)
            t = {fn.__name__: timed(fn) for fn in order}
            if rnd >= 5:
                for key in ts:
                    ts[key].append(t[key])
        # the host plan: the records the device's unwrap would hand back, in order
        cap = 1 << 30
        nplan = int(np.searchsorted(idx, cap, side="right")) - 1 if total > cap else n
        recs = np.zeros(nplan + 1, TCP_RX_DTYPE)
        recs["status"] = 0x0F
        recs["pay_off"][1:], recs["pay_len"][1:] = 40, pl[:nplan]
        recs["msg"]["seqno"][1:] = (ISN + 1 + idx[:nplan]) & 0xFFFFFFFF
        recs["msg"]["seqno"][0], recs["msg"]["flags"][0], recs["pay_off"][0] = ISN, 2, 40  # the SYN, in a 40-byte datagram
        poff = np.concatenate([[0], off[:nplan + 1] + 40]).astype(np.uint64)
        plan_ts = []
        for _ in range(7):
            rx = RxStream(cap)
            out = np.empty(nplan + 1, COPY_PIECE_DTYPE)
            cnt = ctypes.c_uint64()
            t0 = time.perf_counter()
            rc = rx.lib.ics_rx_stream_plan(rx.handle, recs.ctypes.data, len(recs), None, poff.ctypes.data, 0, 0,
                                           out.ctypes.data, len(out), ctypes.byref(cnt))
            plan_ts.append((time.perf_counter() - t0) * 1e6)
            assert rc == 0 and cnt.value == int((pl[:nplan] > 0).sum()) and rx.stats()["bytes_pushed"] == int(idx[nplan])
            rx.close()
        # the feature's own call on the same records, a fresh stream (and ring) per round
        ring_cap = int(idx[nplan])
        rx_ts, rx_host = [], []
        for rnd in range(RX_ROUNDS + 2):
            rx = eng.rx_stream(ring_cap)
            t_host = [0.0]

            def receive():
                t0 = time.perf_counter()
                rx.receive(src_full, recs, offsets=poff)
                t_host[0] = (time.perf_counter() - t0) * 1e6

            t = timed(receive)
            assert eng.dispatch_info()["kernel"] == "copy_pieces" and rx.stats()["bytes_pushed"] == ring_cap
            if rnd == 0:  # the ring holds the payloads in order
                head = np.frombuffer(rx.read(4096), np.uint8)
                want = torch.cat([src[int(off[k]) + 40:int(off[k]) + 40 + int(pl[k])] for k in range(64)])[:4096]
                assert (head == want.cpu().numpy()[:len(head)]).all() and len(head) == min(4096, ring_cap)
            if rnd >= 2:
                rx_ts.append(t)
                rx_host.append(t_host[0])
            rx.close()
        rx_ts.sort()
        rx_host.sort()
        mplan = int((pl[:nplan] > 0).sum())
        row = {"shape": name, "row": "receive_batch", "records": nplan + 1, "pieces": mplan, "bytes": ring_cap,
               "median_us": round(statistics.median(rx_ts), 1), "p10_us": round(rx_ts[len(rx_ts) // 10], 1),
               "p90_us": round(rx_ts[(9 * len(rx_ts)) // 10], 1), "host_call_us": round(statistics.median(rx_host), 1),
               "list_mb": round(16 * mplan / 1e6, 2), "rounds": len(rx_ts)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        traffic = 2 * total + 16 * m
        for key, xs in ts.items():
            xs.sort()
            row = {"shape": name, "row": key, "n": n, "pieces": m, "bytes": total,
                   "median_us": round(statistics.median(xs), 2), "p10_us": round(xs[len(xs) // 10], 2),
                   "p90_us": round(xs[(9 * len(xs)) // 10], 2), "rounds": len(xs),
                   "tb_per_s": round(2 * total / statistics.median(xs) / 1e6, 3)}
            if key == "copy":
                row["traffic_mb"] = round(traffic / 1e6, 1)
                row["floor_us"] = round(traffic / 8e12 * 1e6, 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        plan_ts.sort()
        row = {"shape": name, "row": "plan", "records": nplan + 1, "median_us": round(statistics.median(plan_ts), 1),
               "ns_per_record": round(statistics.median(plan_ts) * 1e3 / (nplan + 1), 1), "rounds": len(plan_ts)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        for row in host_rows(name, n):
            rows.append(row)
            print(json.dumps(row), flush=True)
        del src, src_full, dst, plain, dp
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
