"""CPU tests of the receive streams (include/icsum.h, "receive streams"):
golden/reasm_cases.json — recorded from the real reference's TCPReceiver,
Reassembler and ByteStream (tools/gen_reasm_golden.cpp) — pins the Python
restatement (reasm_ref.py), and both pin the library's stream object, driven
through ics_rx_stream_plan with the pieces applied to a numpy ring, in both
builds.  No GPU is needed.  The inventory entry is README_reasm.md."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from reasm_ref import RefStream
from rx_driver import (ANSWERS, CAPS, ISNS, PlanDriver, lib_answers, load_golden, pack_plain, random_stream, recv,
                       ref_apply, run_scenario)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc")
MERGES = ["touch_prev", "inside_prev", "inside_prev_same_end", "overlap_prev", "same_beg_longer", "same_beg_shorter",
          "duplicate_pending", "next_keeps", "next_covered", "next_touch", "next_same_end", "bridge",
          "bridge_all_covered", "prev_and_next", "first_position", "first_position_overlap"]
TAGS = (["in_order", "reversed", "holes_interleaved"] + [f"merge_{m}_{k}" for m in MERGES for k in ("agree", "conflict")]
        + ["duplicate_pushed", "straddle_unassembled", "edge_straddle", "edge_at", "edge_past", "edge_after_pop",
           "cap1", "cap2", "cap7", "cap65535", "cap70000_window", "wrap_many", "fin_in_order", "fin_early",
           "fin_empty", "fin_empty_early", "fin_duplicated", "fin_moved_earlier", "fin_behind_window",
           "fin_clipped_empty", "data_after_fin", "data_after_close", "syn_with_data", "syn_fin", "syn_fin_data",
           "second_syn", "data_before_syn", "fin_before_syn", "rst_first", "rst_syn_first", "rst_middle",
           "set_error_then_data", "isn_0", "isn_2147483648", "isn_4294967295", "cross_2_32"]
        + [f"half_space_{side}_{d}_pushed{p}" for p in (0, 40) for d in (2**31 - 1, 2**31, 2**31 + 1)
           for side in ("above", "below")]
        + ["seqno_is_isn_no_syn", "seqno_below_isn"])


@pytest.fixture(scope="module")
def gold():
    return load_golden()


@pytest.fixture(scope="module", params=[False, True], ids=["release", "debug"])
def debug(request):
    return request.param


def by_tag(gold, tag):
    return next(s for s in gold if s["tag"] == tag)


def test_fixture_holds_the_cases(gold):
    assert [s["tag"] for s in gold] == TAGS
    assert {s["capacity"] for s in gold} >= {1, 2, 7, 65535}
    ends = lambda tag: by_tag(gold, tag)["ops"][-1]  # noqa: E731
    # what the tags say, from the reference's own answers
    assert ends("fin_in_order")["closed"] and ends("fin_early")["closed"] and ends("fin_empty")["closed"]
    behind = by_tag(gold, "fin_behind_window")["ops"]
    assert not behind[1]["closed"] and not behind[3]["closed"] and behind[3]["pushed"] == 8  # rejected: no eof
    assert behind[-1]["closed"]
    clipped = by_tag(gold, "fin_clipped_empty")["ops"]
    assert not clipped[2]["closed"] and clipped[-2]["closed"] and clipped[-2]["pushed"] == 10  # eof set by an empty clip
    assert ends("rst_first")["error"] and ends("rst_first")["ackno"] is None and ends("rst_first")["rst"]
    assert ends("set_error_then_data")["pushed"] == 4 and ends("rst_middle")["pending"] == 4
    assert by_tag(gold, "data_before_syn")["ops"][1]["ackno"] is None
    assert ends("cap70000_window")["window"] == 65535 and ends("cap70000_window")["avail"] == 70000
    assert ends("cross_2_32")["pushed"] == 605 and ends("cross_2_32")["ackno"] < 1000
    assert ends("seqno_is_isn_no_syn")["pushed"] == 4
    wraps = by_tag(gold, "wrap_many")
    assert wraps["ops"][-1]["pushed"] >= 7 * wraps["capacity"]  # the window wraps the ring several times
    second = by_tag(gold, "second_syn")["ops"]
    assert second[1]["pushed"] == 5 and second[1]["ackno"] == 1006  # inserted at index 0, the ISN kept
    # conflicting bytes: the winner rules are visible in what was popped
    for m in MERGES:
        a, c = (by_tag(gold, f"merge_{m}_{k}")["ops"] for k in ("agree", "conflict"))
        assert [o["pushed"] for o in a] == [o["pushed"] for o in c]
        if m not in ("touch_prev", "next_touch", "first_position"):
            assert a[-1]["popped"] != c[-1]["popped"], m


def test_restatement_reproduces_the_fixture(gold):
    for sc in gold:
        ref = RefStream(sc["capacity"])
        for k, op in enumerate(sc["ops"]):
            out = ref_apply(ref, op)
            if op["op"] == "pop":
                assert out.hex() == op["popped"], (sc["tag"], k)
            assert ref.answers() == {key: op[key] for key in ANSWERS}, (sc["tag"], k)


@pytest.mark.parametrize("how", ["each", "whole", "random"])
def test_library_reproduces_the_fixture(gold, debug, how):
    for i, sc in enumerate(gold):
        for seed in ((1, 2, 3) if how == "random" else (0,)):
            drv = PlanDriver(sc["capacity"], debug=debug, lead=i % 4)
            run_scenario(drv, sc, how, seed=1000 * seed + i)
            drv.close()


# ---- the seeded random run -------------------------------------------------
@pytest.fixture(scope="module")
def random_run():
    """40 streams, 20 000 segments: the operations and, from the restatement
    alone, the expected answers after each and the conditions on the inputs"""
    rng = random.Random(0x7265736D)
    streams, segs, contributed, new_wins, old_keeps = [], 0, 0, 0, 0
    for s in range(40):
        cap, isn = CAPS[s % len(CAPS)], ISNS[(s // 2) % len(ISNS)]
        ops = random_stream(rng, cap, isn, 500)
        ref, want, popped = RefStream(cap), [], 0
        for op in ops:
            out = ref_apply(ref, op)
            if op["op"] == "recv":
                segs += 1
                contributed += ref.contributed
            else:
                popped += len(out)
            want.append((ref.answers(), out, ref.popped, len(ref.bufs), ref.eof))
        assert popped > 0, ("a stream that never reaches a pop", s, cap)
        new_wins += ref.new_wins
        old_keeps += ref.old_keeps
        streams.append((cap, ops, want))
    print(f"segments {segs}, contributing {contributed}, conflicting overlaps new wins {new_wins} / old keeps {old_keeps}")
    assert segs >= 20000
    assert contributed >= segs // 4
    assert new_wins >= 200 and old_keeps >= 200
    return streams


def test_random_streams_restatement_equals_library(random_run, debug):
    cuts = random.Random(5)
    for s, (cap, ops, want) in enumerate(random_run):
        drv = PlanDriver(cap, debug=debug, lead=s % 4)
        k = 0
        while k < len(ops):
            tag = (s, cap, k)
            if ops[k]["op"] == "recv":
                # one record per call on every other stream, random cuts on the rest
                j = k + 1
                while s % 2 and j < len(ops) and ops[j]["op"] == "recv" and cuts.random() < 0.7:
                    j += 1
                drv.batch(ops[k:j], tag)
                k = j
            else:
                assert drv.pop(ops[k]["n"]) == want[k][1], tag
                k += 1
            answers, _, popped, intervals, eof = want[k - 1]
            assert drv.answers() == answers, tag
            st = drv.rx.stats()
            assert (st["bytes_popped"], st["intervals"], st["eof_index"]) == (popped, intervals, eof), tag
        drv.close()


# ---- the ABI ----------------------------------------------------------------
def test_ctypes_mirror_matches_the_header(tmp_path):
    from tcpip_network_protocol_stack_amd import _lib
    from tcpip_network_protocol_stack_amd.engine import COPY_PIECE_DTYPE

    structs = {"ics_copy_piece": _lib.CopyPiece, "ics_rx_send_t": _lib.RxSend, "ics_rx_stats_t": _lib.RxStats}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "icsum.h"', "int main(void) {",
             '  printf("kernel %d\\n", ICS_K_COPY_PIECES);', '  printf("abi %d\\n", ICS_ABI_VERSION);']
    for name, py in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in py._fields_:
            lines.append(f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, py in structs.items():
        assert int(got[name]) == ctypes.sizeof(py), name
        for f, _ in py._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(py, f).offset, (name, f)
    assert int(got["ics_copy_piece"]) == COPY_PIECE_DTYPE.itemsize == 16
    for f, _ in _lib.CopyPiece._fields_:
        assert COPY_PIECE_DTYPE.fields[f][1] == getattr(_lib.CopyPiece, f).offset
    assert int(got["kernel"]) == 23 and _lib.KERNELS[23] == "copy_pieces" and len(_lib.KERNELS) == 23
    assert int(got["abi"]) == 2 and _lib.load().ics_abi_version() == 2


def test_argument_errors(debug):
    from tcpip_network_protocol_stack_amd import _lib
    from tcpip_network_protocol_stack_amd.engine import COPY_PIECE_DTYPE, TCP_RX_DTYPE, RxStream

    lib = _lib.load(_lib.DEBUG_LIB_PATH if debug else None)
    err = lambda: lib.ics_last_error().decode()  # noqa: E731
    h = ctypes.c_void_p()
    for cap in (0, 2**30 + 1, 2**63):
        assert lib.ics_rx_stream_create_host(cap, ctypes.byref(h)) == -1 and h.value is None
        assert "outside 1 .. 2^30" in err()
    assert lib.ics_rx_stream_create_host(8, None) == -1 and "null output" in err()
    rx = RxStream(8, debug=debug)
    ops = [recv(100, b"", syn=True), recv(101, b"abcdef")]
    buf, recs, off, _, _ = pack_plain(ops, TCP_RX_DTYPE, False)
    m = ctypes.c_uint64(77)
    pieces = np.zeros(4, COPY_PIECE_DTYPE)
    before = rx.stats()

    def plan(rxs, r, n, offsets, stride=0, dlen=0, out=pieces, cap=4, count=m):
        return lib.ics_rx_stream_plan(rxs, r.ctypes.data if r is not None else None, n,
                                      None, offsets.ctypes.data if offsets is not None else None, stride, dlen,
                                      out.ctypes.data if out is not None else None, cap,
                                      ctypes.byref(count) if count is not None else None)

    assert plan(None, recs, 2, off) == -1 and "null stream" in err()
    assert plan(rx.handle, None, 2, off) == -1 and "null records" in err()
    assert plan(rx.handle, recs, 2, off, count=None) == -1 and "null piece count" in err()
    bad = off.copy()
    bad[2] = bad[1] - 1
    assert plan(rx.handle, recs, 2, bad) == -1 and "offsets decrease at datagram 1" in err()
    long = recs.copy()
    long[1]["pay_len"] = 7
    assert plan(rx.handle, long, 2, off) == -1 and "record 1: payload [40, 40 + 7) outside its datagram of 46" in err()
    assert plan(rx.handle, long, 2, None, stride=64, dlen=46) == -1 and "outside its datagram" in err()
    assert plan(rx.handle, recs, 2, off, cap=0) == -1 and "holds less than the plan's 1 pieces" in err()
    # nothing above changed the state or the outputs
    assert m.value == 77 and not pieces.view(np.uint8).any() and rx.stats() == before
    assert rx.plan(recs, offsets=off, dry=True) == 1 and rx.stats() == before
    skipped = long.copy()
    skipped[1]["status"] = 0x07  # not PROTO_TCP: not taken, so its payload range is not looked at
    assert len(rx.plan(skipped, offsets=off)) == 0 and rx.stats()["has_isn"] == 1
    got = rx.plan(recs[1:], offsets=off[1:])
    assert got.tolist() == [(int(off[1]) + 40, 0, 6)]
    # pop beyond what is buffered is refused; peek, send and stats want their outputs
    assert lib.ics_rx_stream_pop(rx.handle, 7) == -1 and "pop of 7 bytes with 6 buffered" in err()
    assert lib.ics_rx_stream_send(rx.handle, None) == -1 and lib.ics_rx_stream_stats(None, None) == -1
    assert lib.ics_rx_stream_peek(rx.handle, None, None, None) == -1 and lib.ics_rx_stream_set_error(None) == -1
    assert rx.peek() == [(0, 6)]
    rx.pop(6)
    assert rx.peek() == [] and lib.ics_rx_stream_destroy(None) == 0
    # the device calls check the context first: no GPU is needed to see it
    assert lib.ics_rx_stream_create(None, 8, ctypes.byref(h)) == -1 and "null context" in err()
    assert lib.ics_rx_stream_receive_batch(None, rx.handle, None, None, 0, 0, 1, None, None, None) == -1
    assert "null context" in err()
    got_n = ctypes.c_uint64()
    assert lib.ics_rx_stream_read(None, rx.handle, None, 0, ctypes.byref(got_n), None) == -1 and "null context" in err()
    assert lib.ics_copy_pieces(None, None, 0, None, 0, None, 1, None) == -1 and "null context" in err()
    d = ctypes.c_void_p()
    assert lib.ics_rx_stream_ring(rx.handle, ctypes.byref(d)) == -1 and "without a ring" in err()
    rx.close()


def test_take_array_selects_records(debug):
    from tcpip_network_protocol_stack_amd.engine import TCP_RX_DTYPE, RxStream

    ops = [recv(50, b"", syn=True), recv(51, b"xxxx"), recv(51, b"abcd"), recv(55, b"ef")]
    buf, recs, off, _, _ = pack_plain(ops, TCP_RX_DTYPE, False)
    recs["status"] = 0  # take, not the status, decides
    rx = RxStream(16, debug=debug)
    pieces = rx.plan(recs, take=[1, 0, 1, 1], offsets=off)
    assert pieces.tolist() == [(int(off[2]) + 40, 0, 4), (int(off[3]) + 40, 4, 2)]
    assert lib_answers(rx)["pushed"] == 6
    rx.close()


def test_selftest_under_sanitizers(tmp_path):
    """csrc/tests/rxstream_selftest.cpp: icsum_rxstream.cpp linked alone — the
    merge branches, 100 000 random inserts at capacity 64 against a byte-array
    model, the piece array at its exact capacity — under ASan + UBSan, as a
    child process"""
    exe = tmp_path / "rxstream_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "tests", "rxstream_selftest.cpp"), os.path.join(CSRC, "icsum_rxstream.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert not any(m in r.stderr for m in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))
    assert r.stdout.startswith("rxstream_selftest ok")


@pytest.mark.skipif(not os.path.isdir("/root/reference/src"), reason="needs the reference stack sources")
def test_rx_stream_against_the_reference_receiver():
    """csrc/host/tests/rx_stream_test.cpp: the reference's own TCPReceiver,
    compiled in place on the drop-in headers, against icsum::RxStream::plan on
    the same 6000 mixed wires, segment for segment, the pieces applied on the
    host"""
    host = os.path.join(CSRC, "host")
    subprocess.check_call(["make", "-s", "-j8", "-C", host], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(host, "build", "rx_stream_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-3000:]
    assert out.stdout.startswith("OK:") and "6000 wires" in out.stdout
