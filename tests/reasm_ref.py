"""Python restatement of the receive stream (include/icsum.h, "receive
streams"): TCPReceiver::receive, Wrap32::unwrap, Reassembler::insert and the
writer half of ByteStream, written from the semantics block there, with the
bytes in place (each interval holds a bytearray).  It is the oracle of
test_rx_stream.py and test_gpu_rx_stream.py: golden/reasm_cases.json (recorded
from the real reference) pins it, and it pins the library.

Beside the state it counts, for the random tests' input conditions, the
conflicting overlaps it resolved each way: `new_wins` (overlaps in which bytes
of an earlier interval were replaced by different bytes of the new segment) and
`old_keeps` (overlaps in which bytes of the new segment were dropped in favour
of different bytes already held)."""

M32 = 0xFFFFFFFF
NO_EOF = (1 << 64) - 1


def unwrap(raw, isn, checkpoint):
    """Wrap32::unwrap with the reference's conversions."""
    offset = (raw - ((isn + checkpoint) & M32)) & M32
    if offset >= 1 << 31:
        offset -= 1 << 32  # int32_t
    absseq = (checkpoint + offset) & ((1 << 64) - 1)
    if absseq >= 1 << 63:  # negative as an int64_t: + 2^32
        absseq = (absseq + (1 << 32)) & ((1 << 64) - 1)
    return absseq


class RefStream:
    def __init__(self, capacity):
        self.capacity = capacity
        self.isn = None
        self.pushed = 0  # == first_unassembled_index_
        self.popped = 0
        self.eof = NO_EOF
        self.closed = False
        self.error = False
        self.bufs = []  # [beg, end, bytearray, owners], ordered; owners: the receive() that sent each byte
        self.calls = 0
        self.stream = bytearray()  # the buffered bytes [popped, pushed)
        self.stream_own = []  # ... and the receive() that sent each
        self.new_wins = 0
        self.old_keeps = 0
        self.contributed = False  # did the last receive() keep a byte of its payload?

    # ---- queries ---------------------------------------------------------
    def available(self):
        return self.capacity - (self.pushed - self.popped)

    def pending(self):
        return sum(iv[1] - iv[0] for iv in self.bufs)

    def send(self):
        ack = None if self.isn is None else (self.isn + self.pushed + 1 + (1 if self.closed else 0)) & M32
        return {"ackno": ack, "window": min(self.available(), 65535), "rst": self.error}

    def answers(self):
        """what golden/reasm_cases.json records after every operation"""
        s = self.send()
        return {"pushed": self.pushed, "pending": self.pending(), "avail": self.available(),
                "closed": int(self.closed), "error": int(self.error), "ackno": s["ackno"], "window": s["window"],
                "rst": int(s["rst"])}

    def owned_since(self, call):
        """bytes now held, pending or buffered, that a receive() after call number `call` sent"""
        return sum(1 for o in self.stream_own if o > call) + sum(1 for iv in self.bufs for o in iv[3] if o > call)

    def held(self):
        """[(stream index, bytes)]: everything held — the buffered bytes, then each pending interval"""
        return [(self.popped, bytes(self.stream))] + [(iv[0], bytes(iv[2])) for iv in self.bufs]

    # ---- operations --------------------------------------------------------
    def set_error(self):
        self.error = True

    def pop(self, n):
        """read(reader, n): at most n buffered bytes, popped"""
        n = min(n, len(self.stream))
        out = bytes(self.stream[:n])
        del self.stream[:n]
        del self.stream_own[:n]
        self.popped += n
        return out

    def receive(self, seqno, payload=b"", syn=False, fin=False, rst=False):
        self.contributed = False
        self.calls += 1
        if self.error:
            return
        if rst:
            self.error = True
            return
        if self.isn is None:
            if not syn:
                return
            self.isn = seqno
        absseq = unwrap(seqno, self.isn, self.pushed + 1)
        idx = 0 if syn else (absseq - 1) & ((1 << 64) - 1)
        self._insert(idx, bytes(payload), fin)

    def _insert(self, first, data, last):
        edge = self.pushed + self.available()
        if self.closed or first >= self.eof or first >= edge:
            return
        if last:
            self.eof = first + len(data)
        beg, end = max(first, self.pushed), min(first + len(data), edge)
        if end <= beg:
            if self.pushed >= self.eof:
                self.closed = True
            return
        new = bytearray(data[beg - first:end - first])
        own = [self.calls] * len(new)
        bufs = self.bufs
        # lower_bound by (beg, end)
        it = 0
        while it < len(bufs) and (bufs[it][0], bufs[it][1]) < (beg, end):
            it += 1
        if it == 0:
            bufs.insert(0, [beg, end, new, own])
            cur = 0
            it = 1
        else:
            prev = bufs[it - 1]
            if prev[1] >= beg:  # touching intervals merge
                if prev[1] <= end:  # the new range wins its overlap
                    keep = beg - prev[0]
                    self.new_wins += any(a != b for a, b in zip(prev[2][keep:], new))
                    prev[2] = prev[2][:keep] + new
                    prev[3] = prev[3][:keep] + own
                    prev[1] = end
                else:  # wholly inside: discarded
                    o = beg - prev[0]
                    self.old_keeps += any(a != b for a, b in zip(prev[2][o:o + len(new)], new))
                cur = it - 1
            else:
                bufs.insert(it, [beg, end, new, own])
                cur = it
                it += 1
        c = bufs[cur]
        while it < len(bufs) and c[1] >= bufs[it][0]:
            nx = bufs[it]
            o = nx[0] - c[0]
            if nx[1] > c[1]:  # a following interval that ends later keeps its overlap
                self.old_keeps += any(a != b for a, b in zip(c[2][o:], nx[2]))
                c[2] = c[2][:o] + nx[2]
                c[3] = c[3][:o] + nx[3]
                c[1] = nx[1]
            else:  # covered: erased
                self.new_wins += any(a != b for a, b in zip(c[2][o:o + len(nx[2])], nx[2]))
            del bufs[it]
        self.contributed = self.calls in c[3]
        # push while an interval starts at first_unassembled
        k = 0
        while k < len(bufs):
            if bufs[k][0] == self.pushed:
                self.stream += bufs[k][2]
                self.stream_own += bufs[k][3]
                self.pushed = bufs[k][1]
                del bufs[k]
            else:
                k += 1
        if self.pushed >= self.eof:
            self.closed = True
