"""CPU: the route table (ics_route_table_*, csrc/icsum_route.cpp) against the
real reference's Router::match.

tests/golden/route_cases.json holds the answers of the reference's own
Router::add_route / Router::match (the reference's src/router/router.cpp:15-24,
:77-87; produced by tools/gen_route_golden.cpp) for tables with an empty table,
default routes alive and dead, nested prefixes around every trie level
boundary (/15-/17, /23-/25, /30-/31), overwritten duplicates, a next hop of
0.0.0.0 and routes with host bits set, each probed at every prefix's first,
last, one-before and one-past address with bit 0 either way.  RouteTable.match
— which walks the compiled image the device reads — must give those answers,
and so must the Python restatement (route_ref.py), against which larger random
tables are then checked.  No GPU, no context.  Bar: exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
from route_ref import RefRouter, boundary_addrs, fill, is_live, random_routes

CSRC = os.path.join(ROOT, "tcpip_network_protocol_stack_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    return golden("route_cases.json")["tables"]


def _table():
    from tcpip_network_protocol_stack_amd.engine import RouteTable

    return RouteTable()


def _check(table, ref, addrs):
    for a in addrs:
        assert table.match(int(a)) == ref.answer(int(a)), hex(int(a))


def test_fixture_covers_what_it_should(cases):
    names = {c["name"] for c in cases}
    assert {"empty", "default_alone", "default_nonzero_prefix_is_dead", "nested_15_16_17", "nested_23_24_25",
            "nested_30_31", "duplicates_overwrite", "next_hop_zero_is_not_direct", "host_bits_set_are_dead"} <= names
    for c in cases:
        assert len(c["addrs"]) == len(c["answers"]) >= 20
    assert any(not a[0] for c in cases for a in c["answers"]) and any(a[0] for c in cases for a in c["answers"])
    assert any(a[0] and a[2] and a[3] == 0 for c in cases for a in c["answers"])  # a matched next hop of 0.0.0.0


def test_restatement_equals_the_reference(cases):
    for c in cases:
        ref = RefRouter(c["routes"])
        for addr, (m, iface, has, hop) in zip(c["addrs"], c["answers"]):
            got = ref.match(addr)
            assert (got is not None) == bool(m), (c["name"], addr)
            if m:
                assert got == (iface, bool(has), hop if has else got[2]), (c["name"], addr)
                assert has or got[2] == 0


def test_table_equals_the_reference(cases):
    for c in cases:
        t = fill(_table(), c["routes"])
        for addr, (m, iface, has, hop) in zip(c["addrs"], c["answers"]):
            want = (iface, hop if has else addr) if m else None  # next_hop.value_or(dst)
            assert t.match(addr) == want, (c["name"], addr)
        st = t.stats()
        assert st["routes_added"] == len(c["routes"])
        assert st["routes_live"] == sum(is_live(r[0], r[1]) for r in c["routes"])
        assert st["routes_dead"] == st["routes_added"] - st["routes_live"]
        assert st["route_records"] == len({(r[1], r[0]) for r in c["routes"] if is_live(r[0], r[1])})
        assert st["image_words"] == 65536 + 256 * st["l2_chunks"] + 128 * st["l3_chunks"]
        t.close()


@pytest.mark.parametrize("n", [0, 1, 2, 17, 300, 2000])
def test_random_tables_equal_the_restatement(n):
    rng = np.random.default_rng(0x2007 + n)
    routes = random_routes(rng, n)
    t, ref = fill(_table(), routes), RefRouter(routes)
    addrs = boundary_addrs(routes)[:6000] + [int(a) for a in rng.integers(0, 2**32, 1500)]
    _check(t, ref, addrs)
    st = t.stats()
    assert st["routes_dead"] == sum(not is_live(r[0], r[1]) for r in routes)
    if n >= 300:
        assert st["routes_dead"] > 0 and st["route_records"] < st["routes_live"]  # dead and duplicate routes occurred
        assert st["l2_chunks"] > 0 and st["l3_chunks"] > 0
    t.close()


def test_large_table():
    """50 000 routes, mostly /8../24 with some /25../31: 20 000 addresses
    against the restatement, and the image within 65536 + 256 c2 + 128 c3 words"""
    rng = np.random.default_rng(50_000)
    lengths = list(range(8, 25)) * 6 + list(range(25, 32))
    routes = random_routes(rng, 50_000, lengths=lengths, dead=0.05, dup=0.05)
    # spread: most routes under their own random /16 instead of the few shared bases
    for k in range(0, len(routes), 2):
        p, length, iface, has, hop = routes[k]
        routes[k] = (int(rng.integers(0, 2**32)) & (0xFFFFFFFF << (32 - length)) & 0xFFFFFFFF, length, iface, has, hop)
    t, ref = fill(_table(), routes), RefRouter(routes)
    b = boundary_addrs(routes)
    addrs = [b[int(k)] for k in rng.integers(0, len(b), 14_000)] + [int(a) for a in rng.integers(0, 2**32, 6_000)]
    _check(t, ref, addrs)
    st = t.stats()
    assert st["routes_added"] == 50_000
    assert st["image_words"] <= 65536 + 256 * st["l2_chunks"] + 128 * st["l3_chunks"]
    assert st["l2_chunks"] > 1000 and st["l3_chunks"] > 100
    t.close()


def test_invalid_arguments_have_a_message():
    from tcpip_network_protocol_stack_amd import _lib

    lib = _lib.load()
    t = _table()
    u32 = ctypes.c_uint32

    def invalid(rc, word):
        assert rc == -1, rc
        assert word in lib.ics_last_error().decode(), lib.ics_last_error()

    invalid(lib.ics_route_table_add(t.handle, 0, 32, 0, 0, 0), "32")
    invalid(lib.ics_route_table_add(t.handle, 0, 255, 0, 0, 0), "255")
    invalid(lib.ics_route_table_add(t.handle, 0, 8, 2**31, 0, 0), "2^31")
    invalid(lib.ics_route_table_create(None), "null")
    invalid(lib.ics_route_table_add(None, 0, 8, 0, 0, 0), "null")
    invalid(lib.ics_route_table_clear(None), "null")
    invalid(lib.ics_route_table_match(None, 0, None, None), "null")
    invalid(lib.ics_route_table_stats(t.handle, None), "null")
    invalid(lib.ics_route_table_stats(None, None), "null")
    invalid(lib.ics_route_lookup_batch(None, t.handle, None, 1, None, None, None), "null context")
    with pytest.raises(_lib.IcsumError, match="above 31"):
        t.add(0, 32, 0)
    assert t.stats()["routes_added"] == 0  # a rejected add leaves nothing behind
    assert lib.ics_route_table_add(t.handle, 0x0A000000, 31, 2**31 - 1, 0, 0) == 0
    f, h = u32(), u32()
    assert lib.ics_route_table_match(t.handle, 0x0A000001, ctypes.byref(f), None) == 1 and f.value == 2**31 - 1
    assert lib.ics_route_table_match(t.handle, 0x0A000002, ctypes.byref(f), ctypes.byref(h)) == 0
    assert (f.value, h.value) == (0xFFFFFFFF, 0)
    assert lib.ics_route_table_destroy(None) == 0
    t.close()


def test_clear_then_add_again():
    t = _table()
    t.add(0x0A000000, 8, 1)
    t.add(0x0A010000, 16, 2, next_hop=0)
    t.add(0x0A010001, 16, 3)  # dead
    assert t.match(0x0A010203) == (2, 0) and t.match(0x0A020304) == (1, 0x0A020304) and t.match(0x0B000000) is None
    assert {k: t.stats()[k] for k in ("routes_added", "routes_live", "routes_dead", "route_records")} == \
        {"routes_added": 3, "routes_live": 2, "routes_dead": 1, "route_records": 2}
    t.clear()
    assert t.match(0x0A010203) is None
    st = t.stats()
    assert (st["routes_added"], st["image_words"], st["l2_chunks"]) == (0, 65536, 0)
    t.add(0x0A010200, 24, 7)
    assert t.match(0x0A010203) == (7, 0x0A010203) and t.match(0x0A010303) is None
    assert t.stats()["l2_chunks"] == 1
    t.add(0x0A010200, 24, 8, next_hop=5)  # a match compiled the image; this add recompiles it
    assert t.match(0x0A0102FF) == (8, 5)
    t.close()
    t.close()


def test_selftest_under_asan_ubsan(tmp_path):
    """csrc/tests/route_selftest.cpp: icsum_route.cpp alone (no HIP, no other
    source) against a brute-force scan, built with ASan + UBSan and run as a
    child process of its own."""
    exe = tmp_path / "route_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(CSRC, "tests", "route_selftest.cpp"), os.path.join(CSRC, "icsum_route.cpp"),
                           "-o", str(exe), "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert not any(m in r.stderr for m in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer"))
    assert r.stdout.startswith("route_selftest ok")
