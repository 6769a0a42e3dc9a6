"""NetworkInterface (the reference's src/network_interface/network_interface.cpp)
and the frame side of Router::route restated in Python, on top of route_ref.py:

  classify()    recv_frame's destination filter, type branch and parses: the
                ICS_FR_* bits the kernels and ics_neigh_table_recv_frame write
  RefNeigh      the neighbour table with NeighTable's interface (per-interface
                cache, pending requests, timers), and the image's hash and
                slot count restated (neigh_hash / slots_for)
  Hop           the caller's side over either table: the received-datagram and
                waiting queues, route(), and the frames transmitted
  replay()      one golden scenario (tests/golden/frame_cases.json,
                tools/gen_frame_golden.cpp) through a Hop

The restatement is checked against the real reference's transmitted frames in
test_neigh_table.py; the device is then checked against it."""
import json
import os

from route_ref import RefRouter

FR_RESOLVED, FR_DGRAM, FR_FOR_US, FR_IPV4, FR_ARP, FR_ARP_OK = 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
RT_FORWARD, RT_ROUTED = 0x01, 0x02
ARP_REPLY, ARP_RELEASE, ARP_REQUEST = 0x01, 0x02, 0x04
BROADCAST = b"\xff" * 6
MAP_DEADLINE, REQ_DEADLINE = 30000, 5000

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_cases.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)["scenarios"]


# ---------------------------------------------------------------- parsing --
def header_sum(h):
    """IPv4Header::compute_checksum over 20 header bytes: checksum field zero,
    the reserved flag bit dropped, options never summed"""
    s = 0
    for k in range(0, 20, 2):
        w = h[k] << 8 | h[k + 1]
        if k == 6:
            w &= 0x7FFF
        if k == 10:
            w = 0
        s += w
    s = (s >> 16) + (s & 0xFFFF)
    s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def ipv4_parses(p):
    return len(p) >= 20 and p[0] >> 4 == 4 and (p[0] & 15) >= 5 and header_sum(p) == (p[10] << 8 | p[11])


def arp_parses(p):
    """ARPMessage::parse: 28 bytes and supported()"""
    return (len(p) >= 28 and p[0:2] == b"\x00\x01" and p[2:4] == b"\x08\x00" and p[4] == 6 and p[5] == 4
            and p[6] == 0 and p[7] in (1, 2))


def classify(frame, mac):
    """recv_frame's classification of one frame arriving on an interface whose
    address is `mac` (None: not configured, status 0)"""
    frame = bytes(frame)
    if mac is None or len(frame) < 14 or frame[0:6] not in (BROADCAST, bytes(mac)):
        return 0
    st, p = FR_FOR_US, frame[14:]
    if frame[12:14] == b"\x08\x00":
        st |= FR_IPV4 | (FR_DGRAM if ipv4_parses(p) else 0)
    elif frame[12:14] == b"\x08\x06":
        st |= FR_ARP | (FR_ARP_OK if arp_parses(p) else 0)
    return st


def forward_header(p):
    """Router::route's rewrite of a parsed datagram's header, serialized: ttl - 1,
    the checksum recomputed, the reserved flag bit dropped — 20 bytes; None when
    ttl <= 1"""
    if p[8] <= 1:
        return None
    h = bytearray(p[:20])
    h[6] &= 0x7F
    h[8] -= 1
    c = header_sum(h)
    h[10], h[11] = c >> 8, c & 0xFF
    return bytes(h)


def arp_frame(mac, ip, opcode, target_ip, target_mac=None):
    """make_frame(TYPE_ARP, serialize(make_arp_mesg(...)), dst)"""
    return ((target_mac or BROADCAST) + mac + b"\x08\x06" + b"\x00\x01\x08\x00\x06\x04" + opcode.to_bytes(2, "big")
            + mac + ip.to_bytes(4, "big") + (target_mac or bytes(6)) + target_ip.to_bytes(4, "big"))


# ------------------------------------------------------------- the table ---
def neigh_hash(iface, ip):
    """csrc/icsum_neigh.h neigh_hash"""
    h = (ip ^ (iface * 0x9E3779B1)) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def slots_for(mappings):
    n = 4
    while n < 2 * mappings:
        n <<= 1
    return n


class RefNeigh:
    """NeighTable's interface over plain dicts, with the reference's rules"""

    def __init__(self):
        self.ident = {}   # iface -> (mac, ip)
        self.maps = {}    # iface -> {ip: [mac, timer]}
        self.reqs = {}    # iface -> {ip: timer (uint32)}
        self.changes = 0  # counts what must bump the engine's generation

    def set_iface(self, iface, mac, ip):
        if self.ident.get(iface) != (bytes(mac), ip):
            self.changes += 1
        self.ident[iface] = (bytes(mac), ip)

    def learn(self, iface, ip, mac):
        m = self.maps.setdefault(iface, {})
        if ip not in m or m[ip][0] != bytes(mac):
            self.changes += 1
        m[ip] = [bytes(mac), 0]

    def lookup(self, iface, ip):
        e = self.maps.get(iface, {}).get(ip)
        return e[0] if e else None

    def tick(self, ms, iface=0xFFFFFFFF):
        for f in (set(self.maps) | set(self.reqs)) if iface == 0xFFFFFFFF else [iface]:
            m = self.maps.get(f, {})
            for ip in list(m):
                m[ip][1] += ms
                if m[ip][1] > MAP_DEADLINE:
                    del m[ip]
                    self.changes += 1
            r = self.reqs.get(f, {})
            for ip in list(r):
                r[ip] = (r[ip] + ms) & 0xFFFFFFFF
                if r[ip] > REQ_DEADLINE:
                    del r[ip]

    def recv_frame(self, iface, frame):
        frame = bytes(frame)
        mac, my_ip = self.ident[iface]
        st = classify(frame, mac)
        ev, sip, reply = 0, 0, None
        if st & FR_ARP_OK:
            p = frame[14:]
            opcode, smac, sip = p[7], p[8:14], int.from_bytes(p[14:18], "big")
            self.learn(iface, sip, smac)
            if opcode == 1 and int.from_bytes(p[24:28], "big") == my_ip:
                ev, reply = ARP_REPLY, arp_frame(mac, my_ip, 2, sip, smac)
            elif opcode == 2:
                ev = ARP_RELEASE
        return st, ev, sip, reply

    def resolve(self, iface, next_hop):
        if iface not in self.ident:
            return None, None
        mac, my_ip = self.ident[iface]
        hit = self.lookup(iface, next_hop)
        if hit is not None:
            return hit + mac + b"\x08\x00", None
        r = self.reqs.setdefault(iface, {})
        if next_hop in r:
            return None, None
        r[next_hop] = 0
        return None, arp_frame(mac, my_ip, 1, next_hop)

    def stats(self):
        n = sum(len(m) for m in self.maps.values())
        used = list(self.ident) + [f for f, m in self.maps.items()]
        return {"ifaces": len(self.ident), "mappings": n, "pending_requests": sum(len(r) for r in self.reqs.values()),
                "image_ifaces": max(used) + 1 if used else 0, "image_slots": slots_for(n)}

    def entries(self):
        return {(f, ip): e[0] for f, m in self.maps.items() for ip, e in m.items()}


# ---------------------------------------------------------- the caller side --
class Hop:
    """The caller's half of the hop over a table with NeighTable's interface:
    datagrams_received per interface, the waiting queue (the reference's
    unordered_multimap releases the entries of one address newest first under
    libstdc++, which the golden fixture records), and the frames sent."""

    def __init__(self, table, n_ifaces, routes=()):
        self.table, self.router = table, RefRouter(routes)
        self.queues = [[] for _ in range(n_ifaces)]
        self.waiting = [[] for _ in range(n_ifaces)]  # (next_hop, serialized datagram)
        self.tx = []

    def take_tx(self):
        out, self.tx = self.tx, []
        return out

    def recv(self, iface, frame):
        st, ev, sip, reply = self.table.recv_frame(iface, frame)
        if st & FR_DGRAM:
            self.queues[iface].append(bytes(frame[14:]))
        if ev & ARP_REPLY:
            self.tx.append((iface, reply))
        if ev & ARP_RELEASE:
            held = [w for w in self.waiting[iface] if w[0] == sip]
            self.waiting[iface] = [w for w in self.waiting[iface] if w[0] != sip]
            for _, wire in reversed(held):
                hdr, _ = self.table.resolve(iface, sip)
                self.tx.append((iface, hdr + wire))
        return st

    def send(self, iface, wire, next_hop):
        """send_datagram of an already serialized datagram"""
        hdr, request = self.table.resolve(iface, next_hop)
        if hdr is not None:
            self.tx.append((iface, hdr + wire))
            return
        self.waiting[iface].append((next_hop, wire))
        if request is not None:
            self.tx.append((iface, request))

    def route(self):
        for q in self.queues:
            while q:
                p = q.pop(0)
                hdr = forward_header(p)
                if hdr is None:
                    continue
                hit = self.router.answer(int.from_bytes(p[16:20], "big"))
                if hit is not None:
                    self.send(hit[0], hdr + p[4 * (p[0] & 15):], hit[1])


def serialized(dgram):
    """serialize(InternetDatagram) of parsed wire bytes: the 20 header bytes with
    the reserved flag bit dropped and the checksum as given, then the payload
    after the options"""
    h = bytearray(dgram[:20])
    h[6] &= 0x7F
    return bytes(h) + bytes(dgram[4 * (dgram[0] & 15):])


def configure(table, scenario):
    for k, (mac, ip) in enumerate(scenario["ifaces"]):
        table.set_iface(k, bytes.fromhex(mac), ip)
    return table


def replay(scenario, table, on_route=None):
    """run every event of a golden scenario; yields (event, transmitted frames,
    queue lengths).  on_route(hop, burst) is called before each route() with the
    recv events since the last one."""
    hop = Hop(configure(table, scenario), len(scenario["ifaces"]), [tuple(r) for r in scenario["routes"]])
    burst = []
    for ev in scenario["events"]:
        if ev["op"] == "recv":
            hop.recv(ev["iface"], bytes.fromhex(ev["frame"]))
            burst.append(ev)
        elif ev["op"] == "tick":
            table.tick(ev["ms"], 0xFFFFFFFF if ev["iface"] < 0 else ev["iface"])
        elif ev["op"] == "send":
            hop.send(ev["iface"], serialized(bytes.fromhex(ev["dgram"])), ev["next_hop"])
        else:
            if on_route:
                on_route(hop, burst)
            burst = []
            hop.route()
        yield ev, hop.take_tx(), [len(q) for q in hop.queues]
