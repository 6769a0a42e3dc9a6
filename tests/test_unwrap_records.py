"""CPU: the ics_tcp_rx record (include/icsum.h) against the real reference.

tests/golden/unwrap_cases.json was written by tools/gen_unwrap_golden.cpp,
linked against the reference's own IPv4Datagram / TCPSegment parsers and
TCPOverIPv4Adapter: per wire datagram whether each parse succeeded and, where
both did, every field and the payload; per adapter scenario whether
unwrap_tcp_in_ip returned a message.  The Python restatement (unwrap_ref.py)
and ics_tcp_unwrap_one from both library builds must say the same, field for
field; random datagrams are then checked between the two, the wrap fixture's
wires must survive unwrap -> wrap, and the host restatement runs alone under
ASan + UBSan.  No GPU, no context.  Bar: exact."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import ROOT, golden
from unwrap_ref import (PARSED, REC, ST_IPV4_OK, ST_PROTO_TCP, TCP_ACK, TCP_FIN, TCP_RST, TCP_SYN, RefAdapter,
                        canonical, fields, fold, header_checksum, load_golden, unwrap, wrap40)

CSRC = os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc")

TAGS = ["len_0", "len_19", "len_20", "len_39", "len_40", "len_41_odd_payload", "len_42_even_payload", "len_1500",
        "hlen_6", "hlen_15", "hlen_15_len_60", "hlen_6_len_43", "version_6", "hlen_4", "bad_ip_checksum",
        "bad_tcp_checksum", "proto_17_verifies", "doff_4", "doff_6", "doff_15", "doff_15_exact_end",
        "doff_15_past_end", "flags_ff", "flags_00_ackno_on_wire", "urgent_nonzero", "tos_nonzero", "fragment_mf",
        "payload_odd_333", "payload_even_1000", "trailing_beyond_len"]


@pytest.fixture(scope="module")
def gold():
    return load_golden()


def lib_unwrap(lib, wire):
    """ics_tcp_unwrap_one's record as its 40 bytes"""
    from tcpip_network_protocol_stack_amd import _lib

    rec = _lib.TcpRx()
    ctypes.memset(ctypes.byref(rec), 0xA5, 40)
    assert lib.ics_tcp_unwrap_one(bytes(wire), len(wire), ctypes.byref(rec)) == 0
    return bytes(rec)


def implementations():
    from tcpip_network_protocol_stack_amd import _lib

    rel, dbg = _lib.load(), _lib.load(_lib.DEBUG_LIB_PATH)
    return [("restatement", unwrap), ("libicsum", lambda w: lib_unwrap(rel, w)),
            ("libicsum_debug", lambda w: lib_unwrap(dbg, w))]


def test_fixture_has_every_case(gold):
    tags = [c["tag"] for c in gold["cases"]]
    assert len(tags) == len(set(tags))
    assert not [t for t in TAGS if t not in tags]
    by = {c["tag"]: c for c in gold["cases"]}
    # the cases are what their tags say, from the reference's own verdicts
    for t in ("len_0", "len_19", "version_6", "hlen_4", "bad_ip_checksum"):
        assert not by[t]["ip_parse_ok"], t
    for t in ("len_20", "len_39", "hlen_15_len_60", "hlen_6_len_43", "bad_tcp_checksum", "doff_4"):
        assert by[t]["ip_parse_ok"] and not by[t]["tcp_parse_ok"], t
    for t in ("len_40", "len_1500", "hlen_6", "hlen_15", "doff_6", "doff_15", "doff_15_exact_end", "doff_15_past_end",
              "flags_ff", "flags_00_ackno_on_wire", "urgent_nonzero", "tos_nonzero", "fragment_mf",
              "trailing_beyond_len", "proto_17_verifies"):
        assert by[t]["ip_parse_ok"] and by[t]["tcp_parse_ok"], t
    assert by["proto_17_verifies"]["proto"] == 17
    assert by["doff_15_past_end"]["payload"] == "" and by["doff_15_exact_end"]["payload"] == ""
    assert not by["flags_00_ackno_on_wire"]["has_ack"] and bytes.fromhex(by["flags_00_ackno_on_wire"]["wire"])[28:32] != b"\0" * 4
    assert len(bytes.fromhex(by["payload_odd_333"]["payload"])) == 333
    assert [len(bytes.fromhex(by[t]["wire"])) for t in ("len_0", "len_19", "len_20", "len_39", "len_40",
                                                        "len_41_odd_payload", "len_1500", "hlen_15_len_60",
                                                        "hlen_6_len_43")] == [0, 19, 20, 39, 40, 41, 1500, 60, 43]
    names = {s["name"] for s in gold["scenarios"]}
    assert {"listening_connects_on_third", "listening", "connected"} <= names


def test_records_match_the_reference_parses(gold):
    for name, fn in implementations():
        for c in gold["cases"]:
            wire = bytes.fromhex(c["wire"])
            rec = fn(wire)
            r = fields(rec)
            where = (name, c["tag"])
            parsed = r["status"] & PARSED == PARSED
            assert bool(r["status"] & ST_IPV4_OK) == c["ip_parse_ok"], where
            if c["ip_parse_ok"]:
                assert parsed == c["tcp_parse_ok"], where
                assert bool(r["status"] & ST_PROTO_TCP) == (c["proto"] == 6), where
            else:
                assert not parsed, where
            assert rec[37:40] == b"\0\0\0" and r["reserved"] == 0, where
            if not parsed:
                assert rec[:36] == b"\0" * 36, where
                continue
            flags = (TCP_ACK if c["has_ack"] else 0) | (TCP_SYN if c["syn"] else 0) | (TCP_FIN if c["fin"] else 0) | \
                (TCP_RST if c["rst"] else 0)
            want = {"src": c["src"], "dst": c["dst"], "ttl": c["ttl"], "id": c["id"], "src_port": c["src_port"],
                    "dst_port": c["dst_port"], "seqno": c["seqno"], "ackno": c["ackno"], "flags": flags,
                    "window": c["window"]}
            assert {k: r[k] for k in want} == want, where
            assert wire[r["pay_off"]:r["pay_off"] + r["pay_len"]].hex() == c["payload"], where
            assert r["pay_off"] + r["pay_len"] == len(wire), where


def test_gates_reproduce_the_adapter(gold):
    for name, fn in implementations():
        for s in gold["scenarios"]:
            a = RefAdapter(s["listening"], s["source"], s["destination"])
            for g in s["dgrams"]:
                assert a.accept(fn(bytes.fromhex(g["wire"]))) == g["unwrap_ok"], (name, s["name"], g["tag"])
            assert a.listening == s["end_listening"], (name, s["name"])
            assert list(a.destination) == s["end_destination"], (name, s["name"])
    # the scenarios are the ones asked for: the third datagram connects a listening adapter ...
    third = next(s for s in gold["scenarios"] if s["name"] == "listening_connects_on_third")
    assert [g["unwrap_ok"] for g in third["dgrams"]][:5] == [False, False, True, True, False]
    # ... and a connected one drops each wrong gate in turn
    conn = {g["tag"]: g["unwrap_ok"] for g in next(s for s in gold["scenarios"] if s["name"] == "connected")["dgrams"]}
    assert conn["passes"] and not any(conn[t] for t in ("wrong_src", "wrong_dst", "wrong_sport", "wrong_dport",
                                                         "wrong_proto"))


def random_datagram(rng):
    """random bytes with, mostly, a header drawn from the fixture's edge values
    and (for a share of them) both checksums fixed up"""
    n = rng.choice([0, 19, 20, 39, 40, 41, 59, 60, 61, 64, 200]) if rng.random() < 0.3 else rng.randrange(0, 201)
    d = bytearray(rng.randbytes(n))
    if n < 20 or rng.random() < 0.1:
        return bytes(d)
    hlen = rng.choice([5, 5, 5, 5, 6, 15, 4])
    d[0] = (rng.choice([4, 4, 4, 4, 4, 4, 4, 6]) << 4) | hlen
    d[9] = rng.choice([6, 6, 6, 6, 17])
    if rng.random() < 0.8:
        d[2:4] = (n & 0xFFFF).to_bytes(2, "big")
    t = min(max(4 * hlen, 20), n)
    if n - t >= 14:
        d[t + 12] = (rng.choice([5, 5, 5, 5, 6, 15, 4]) << 4) | rng.randrange(16)
        d[t + 13] = rng.choice([0x00, 0x10, 0x02, 0x12, 0x11, 0x04, 0x14, 0xFF, rng.randrange(256)])
    if rng.random() < 0.85:  # both checksums fixed up
        if n - t >= 18:
            d[t + 16:t + 18] = b"\0\0"
            be16 = lambda k: d[k] << 8 | d[k + 1]  # noqa: E731
            s = be16(12) + be16(14) + be16(16) + be16(18) + d[9] + ((be16(2) - 4 * hlen) & 0xFFFF)
            s += 256 * sum(d[t::2]) + sum(d[t + 1::2])
            d[t + 16:t + 18] = fold(s).to_bytes(2, "big")
        d[10:12] = header_checksum(d).to_bytes(2, "big")
    return bytes(d)


def test_random_datagrams_restatement_equals_library():
    from tcpip_network_protocol_stack_amd import _lib

    rng = random.Random(0x756E7772)
    wires = [random_datagram(rng) for _ in range(20000)]
    want = [unwrap(w) for w in wires]
    parsed = sum(1 for r in want if r[36] & PARSED == PARSED)
    classes = {r[36] for r in want}
    print(f"parsed {parsed} of {len(wires)}, status classes {sorted(classes)}")
    assert parsed >= len(wires) // 4
    assert len(classes) >= 8
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = _lib.load(path)
        for i, w in enumerate(wires):
            assert lib_unwrap(lib, w) == want[i], (path, i, w.hex())


def test_wrap_fixture_round_trips():
    """every `wrap` case of tcp_wrap.json (the reference's own
    serialize(wrap_tcp_in_ip(msg))) is canonical; its record and payload,
    serialized by the host wrap, reproduce the wire"""
    cases = [c for c in golden("tcp_wrap.json")["cases"] if c["tag"] == "wrap"]
    assert len(cases) == 160
    for name, fn in implementations():
        for c in cases:
            wire = bytes.fromhex(c["wire"])
            assert canonical(wire), c
            r = fields(fn(wire))
            assert r["status"] == 0x0F
            payload = wire[r["pay_off"]:r["pay_off"] + r["pay_len"]]
            assert len(payload) == c["payload_len"] and r["pay_off"] == 40
            assert (r["src"], r["dst"], r["src_port"], r["dst_port"], r["seqno"], r["ackno"], r["window"]) == \
                (c["src"], c["dst"], c["sport"], c["dport"], c["seqno"], c["ackno"] if c["has_ack"] else 0, c["window"])
            assert wrap40(r, payload) + payload == wire, (name, c["wire"][:80])


def test_ctypes_mirror_matches_the_header(tmp_path):
    from tcpip_network_protocol_stack_amd import _lib
    from tcpip_network_protocol_stack_amd.engine import TCP_RX_DTYPE

    py = _lib.TcpRx
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "icsum.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(ics_tcp_rx));', '  printf("msgsize %zu\\n", sizeof(ics_tcp_msg));',
             '  printf("kernel %d\\n", ICS_K_UNWRAP);']
    for f, _ in py._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(ics_tcp_rx, {f}));')
    for f, _ in _lib.TcpMsg._fields_:
        lines.append(f'  printf("msg.{f} %zu\\n", offsetof(ics_tcp_rx, msg.{f}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(py) == TCP_RX_DTYPE.itemsize == REC.size == 40
    assert int(got["msgsize"]) == ctypes.sizeof(_lib.TcpMsg) == 28
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset == TCP_RX_DTYPE.fields[f][1], f
    for f, _ in _lib.TcpMsg._fields_:
        assert int(got[f"msg.{f}"]) == getattr(_lib.TcpMsg, f).offset, f
    assert _lib.KERNELS[int(got["kernel"])] == "unwrap" and int(got["kernel"]) == 22
    assert _lib.load().ics_abi_version() == 2


def test_module_level_unwrap_one(gold):
    from tcpip_network_protocol_stack_amd.engine import tcp_unwrap_one

    wire = bytes.fromhex(next(c for c in gold["cases"] if c["tag"] == "len_1500")["wire"])
    assert bytes(tcp_unwrap_one(wire)) == unwrap(wire)
    assert tcp_unwrap_one(b"").status == 0


def test_argument_errors():
    from tcpip_network_protocol_stack_amd import _lib

    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = _lib.load(path)
        rec = _lib.TcpRx()
        assert lib.ics_tcp_unwrap_one(b"\x45" * 40, 40, None) == -1
        assert b"null record" in lib.ics_last_error()
        assert lib.ics_tcp_unwrap_one(None, 40, ctypes.byref(rec)) == -1
        assert b"null datagram" in lib.ics_last_error()
        assert lib.ics_tcp_unwrap_one(None, 0, ctypes.byref(rec)) == 0 and bytes(rec) == b"\0" * 40
        # the batch calls check the context first: no GPU is needed to see it
        assert lib.ics_tcp_unwrap_batch(None, None, None, 0, 0, 1, None, None, None) == -1
        assert b"null context" in lib.ics_last_error()
        assert lib.ics_tcp_unwrap_batch_host(None, None, None, 0, 0, 1, None) == -1
        assert b"null context" in lib.ics_last_error()


def test_selftest_under_sanitizers(tmp_path):
    """csrc/tests/unwrap_selftest.cpp: icsum_unwrap.cpp linked alone, every
    length 0..130 at the end of an exactly sized heap block, start alignments
    +0..+3, under ASan + UBSan, as a child process"""
    exe = tmp_path / "unwrap_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "tests", "unwrap_selftest.cpp"), os.path.join(CSRC, "icsum_unwrap.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert not any(m in r.stderr for m in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))
    assert r.stdout.startswith("unwrap_selftest ok")
