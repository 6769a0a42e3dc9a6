"""Router::add_route / Router::match (the reference's src/router/router.cpp:15-24,
:77-87) restated in Python, and the table generators the route tests share.

The restatement is checked against the real reference's answers
(tests/golden/route_cases.json, tools/gen_route_golden.cpp) in
test_route_table.py; the larger random tables are then checked against it."""
import numpy as np

NO_ROUTE = 0xFFFFFFFF


def _rotr(x, r):
    r &= 31
    return ((x >> r) | (x << (32 - r))) & 0xFFFFFFFF if r else x


class RefRouter:
    """routes: (prefix, prefix_len, iface, has_next_hop, next_hop) in add order"""

    def __init__(self, routes=()):
        self.table = [dict() for _ in range(32)]
        for r in routes:
            self.add(*r)

    def add(self, prefix, length, iface, has_next_hop, next_hop):
        # routing_table_[L][rotr(prefix, 32 - L)] = {iface, next_hop}: a later add overwrites
        self.table[length][_rotr(prefix, 32 - length)] = (iface, bool(has_next_hop), next_hop)

    def match(self, addr):
        """(iface, has_next_hop, next_hop) of the first hit from L = 31 down, or None"""
        for length in range(31, -1, -1):
            addr >>= 1
            hit = self.table[length].get(addr)
            if hit is not None:
                return hit
        return None

    def answer(self, addr):
        """(iface, next_hop.value_or(addr)) or None: what the engine reports"""
        hit = self.match(addr)
        if hit is None:
            return None
        return hit[0], hit[2] if hit[1] else addr

    def answers(self, addrs):
        """(matched bool array, iface u32 array, next_hop u32 array) with the
        engine's no-route values (0xFFFFFFFF, 0)"""
        n = len(addrs)
        m, f, h = np.zeros(n, dtype=bool), np.full(n, NO_ROUTE, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        for k, a in enumerate(addrs):
            got = self.answer(int(a))
            if got is not None:
                m[k], f[k], h[k] = True, got[0], got[1]
        return m, f, h


def mask_of(length):
    return 0 if length == 0 else (0xFFFFFFFF << (32 - length)) & 0xFFFFFFFF


def boundary_addrs(routes):
    """each route's first, last, one-before and one-past address (of the range
    it would cover with its host bits clear) and its raw prefix, each also with
    bit 0 flipped"""
    out = []
    for prefix, length, *_ in routes:
        m = mask_of(length)
        first = prefix & m
        last = first | (~m & 0xFFFFFFFF)
        for a in (first, last, (first - 1) & 0xFFFFFFFF, (last + 1) & 0xFFFFFFFF, prefix):
            out += [a, a ^ 1]
    return out


def random_routes(rng, n, lengths=None, dead=0.15, dup=0.15):
    """n routes whose prefixes come from a few bases (so they nest), about
    `dead` of them with a host bit set and `dup` repeating an earlier key"""
    bases = [int(b) for b in rng.integers(0, 2**32, 4)] + [0x0A000000 | int(rng.integers(0, 2**16))]
    routes = []
    for _ in range(n):
        length = int(rng.integers(0, 32)) if lengths is None else int(rng.choice(lengths))
        base = bases[int(rng.integers(0, len(bases)))]
        if rng.random() < 0.4:
            base ^= int(rng.integers(0, 2**18))
        prefix = base & mask_of(length)
        if rng.random() < dead:
            prefix |= 1 << int(rng.integers(0, 32 - length))
        if routes and rng.random() < dup:
            prefix, length = routes[int(rng.integers(0, len(routes)))][:2]
        has = bool(rng.integers(0, 2))
        hop = (0 if rng.random() < 0.2 else int(rng.integers(0, 2**32))) if has else 0
        routes.append((prefix, length, int(rng.integers(0, 2**31)), has, hop))
    return routes


def is_live(prefix, length):
    return prefix == 0 if length == 0 else prefix & ~mask_of(length) & 0xFFFFFFFF == 0


def fill(table, routes):
    for prefix, length, iface, has, hop in routes:
        table.add(prefix, length, iface, hop if has else None)
    return table
