"""Builders of the protocol check's test cases (tests/test_proto_host.py on the CPU,
tests/test_gpu_proto.py on the GPU): frames as bytes, batches of segments decoded by the decode
oracle, the directed RFC 6455 table with its hand-written codes, the tile-edge scripts and the
seeded random cases with their coverage count. Expected values never come from here: they are
the table's literals or proto_oracle.check()."""
import numpy as np

import proto_oracle as P
from oracle_lib import oracle_segments

PAD = 32                                                  # WEBSOCKET_BATCH_PAD
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])                     # RFC 6455 5.7's example key
CONT, TEXT, BIN, CLOSE, PING, PONG = 0, 1, 2, 8, 9, 10
NO_BODY = (1 << 64) - 1                                   # the data_off of a frame without a body


def frame(op, body=b"", fin=1, rsv=0, masked=True, key=KEY):
    """one frame's wire bytes: first byte fin | rsv (0x40 / 0x20 / 0x10) | op"""
    n = len(body)
    m = 0x80 if masked else 0
    h = bytes([(0x80 if fin else 0) | rsv | op])
    if n < 126:
        h += bytes([m | n])
    elif n <= 0xFFFF:
        h += bytes([m | 126]) + n.to_bytes(2, "big")
    else:
        h += bytes([m | 127]) + n.to_bytes(8, "big")
    if not masked:
        return h + bytes(body)
    return h + key + bytes(b ^ key[i & 3] for i, b in enumerate(body))


def close(code=None, reason=b"", **kw):
    return frame(CLOSE, (b"" if code is None else code.to_bytes(2, "big")) + reason, **kw)


class Batch:
    """segments laid one after the other (a gap of `gap` bytes before each), decoded by the decode
    oracle: .raw the wire as received, .dec the wire after the in-place decode, .desc / .res what
    every decode entry point reports for it"""

    def __init__(self, segs, max_frames, gap=0):
        parts, self.seg_off, self.seg_len, pos = [], [], [], 0
        for frames in segs:
            b = b"".join(frames)
            parts.append(b"\xA5" * gap + b)
            self.seg_off.append(pos + gap)
            self.seg_len.append(len(b))
            pos += gap + len(b)
        self.raw = np.frombuffer(b"".join(parts) + b"\x5A" * PAD, np.uint8).copy()
        self.dec = self.raw.copy()
        self.max_frames = max_frames
        self.nseg = len(segs)
        self.desc, res = oracle_segments(self.dec, self.seg_off, self.seg_len, max_frames)
        self.res = res.copy()

    def unconsume_last(self, s, status):
        """turn segment s's last frame into the frame that stopped it: counted, not consumed (what
        WEBSOCKET_SEG_ERR_CACHE_OVERFLOW leaves; with status -1, WEBSOCKET_SEG_ERR_DECODE's
        negative ret)"""
        n = int(self.res[s]["n_frames"])
        d = self.desc[s * self.max_frames + n - 1]
        self.res[s]["consumed"] -= int(d["ret"])
        self.res[s]["status"] = status
        if status == -1:
            d["ret"] = -2147483640                            # (int)(14 + 2^31 + 4): websocketframe.c:164
            d["datalen"] = (1 << 31) + 4

    def expect(self, flags=0, rsv_allowed=0, limit=0, state=None):
        wire = self.raw if flags & P.WIRE_MASKED else self.dec
        return P.check(wire, self.seg_off, self.desc, self.res, self.max_frames, flags, rsv_allowed, limit, state)


class Tiled:
    """nseg segments: the segments of the Batch `p`, one period, laid end to end again and again
    and cut after nseg. A Batch's attributes, made by numpy from p's (a descriptor's offsets move
    with its copy of the wire), so that a batch too large for the per-frame builders and oracles
    costs one period of them. tile() repeats any per-segment array of the period the same way;
    expect() is the period's oracle answer repeated, which is exact as long as no state is carried
    in: every segment then stands alone."""

    def __init__(self, p, nseg):
        self.p, self.nseg, self.max_frames = p, nseg, p.max_frames
        self.reps = -(-nseg // p.nseg)
        span = len(p.raw) - PAD                               # one period's wire
        self.raw = np.concatenate([np.tile(p.raw[:span], self.reps), p.raw[span:]])
        self.dec = np.concatenate([np.tile(p.dec[:span], self.reps), p.dec[span:]])
        base = np.repeat(np.arange(self.reps, dtype=np.uint64) * np.uint64(span), p.nseg)[:nseg]   # each segment's copy
        self.seg_off = self.tile(np.asarray(p.seg_off, np.uint64)) + base
        self.seg_len = self.tile(np.asarray(p.seg_len, np.uint64))
        self.res = self.tile(p.res)
        self.desc = self.tile(p.desc, p.max_frames)
        counted = (np.arange(p.max_frames)[None, :] < self.res["n_frames"][:, None]).reshape(-1)
        move = np.repeat(base, p.max_frames) * counted.astype(np.uint64)
        self.desc["frame_off"] += move
        self.desc["data_off"] += move * (self.desc["data_off"] != np.uint64(NO_BODY)).astype(np.uint64)

    def tile(self, a, per=1):
        """an array of the period with `per` entries a segment, for the nseg segments"""
        return np.tile(a, self.reps)[:self.nseg * per].copy()

    def expect(self, flags=0, rsv_allowed=0, limit=0, state=None):
        assert state is None or not np.any(state)
        codes, res, words = self.p.expect(flags, rsv_allowed, limit, None if state is None else np.zeros(self.p.nseg, np.uint64))
        return self.tile(codes, self.max_frames), self.tile(res), None if words is None else self.tile(words)


def one_frame_period():
    """seven segments that count one frame under max_frames 1: a message left open (its second
    frame is cut off by max_frames), a continuation of nothing, a CLOSE with a status that may not
    be sent, pings with and without a body, a message, a CLOSE"""
    return [[frame(TEXT, b"a", fin=0), frame(CONT, b"b")], [frame(CONT, b"c")], [close(1005)], [frame(PING, b"pq")],
            [frame(BIN, b"xyz")], [close(1000, b"bye")], [frame(PING)]]


def long_period():
    """six segments of 765 to 769 frames (4607 in all: the period moves by 255 list positions), each
    three tiles long and more, whose answers need what the tiles before bring along: a message of
    769 one-byte fragments (a limit of 700 bytes stops its frame 700), a message left open over
    500 frames that a TEXT frame then interrupts, a CLOSE at frame 400 with pings before and after
    it, a segment that ends inside a message, a CLOSE with status 1005 as the last of 769 frames,
    a quiet one"""
    text = [frame(TEXT, b"a", fin=0)] + [frame(CONT, b"b", fin=0) for _ in range(768)]
    return [text, quiet(500, tail_open=True) + [frame(PING, b"still open"), error_frame(9, True, 0)] + quiet(266),
            quiet(400) + [close(1000)] + quiet(367) + [close(1005)], quiet(767, tail_open=True), quiet(768) + [close(1005)],
            quiet(765)]


# ---------------------------------------------------------------------------------------------
# The directed table: Autobahn sections 2 (pings), 3 (reserved bits), 4 (opcodes), 5
# (fragmentation) and 7 (close) as frames, one connection per row:
# (name, frames, flags, rsv_allowed, hand-written codes, first_bad, code, close_status, close_frame)
N = P.NONE
EM, EU = P.EXPECT_MASKED, P.EXPECT_UNMASKED
A = P.AFTER_CLOSE


def directed_table():
    t = []

    def row(name, frames, codes, flags=EM, rsv=0):
        bad = [k for k, c in enumerate(codes) if 1 <= c <= 10]
        cl = [k for k, f in enumerate(frames) if f[0] & 15 == 8]
        cf = cl[0] if cl else N
        t.append((name, frames, flags, rsv, codes, bad[0] if bad else N, codes[bad[0]] if bad else 0,
                  (1009 if codes[bad[0]] == 10 else 1002) if bad else 0, cf))

    hello = frame(TEXT, b"Hel")
    # 2: pings
    row("2.1 ping empty", [frame(PING)], [0])
    row("2.5 ping 125", [frame(PING, b"\xfe" * 125)], [0])
    row("2.6 ping 126", [frame(PING, b"\xfe" * 126), hello], [5, 0])
    row("2.7 pong unsolicited", [frame(PONG), frame(PONG, b"abc")], [0, 0])
    row("2.x ping fragmented", [frame(PING, b"a", fin=0), frame(CONT, b"b")], [4, 8])
    row("2.x pong 126 fragmented: the first rule", [frame(PONG, b"x" * 126, fin=0)], [4])
    # 3: reserved bits
    for name, bit in (("RSV1", 0x40), ("RSV2", 0x20), ("RSV3", 0x10)):
        row("3 %s alone" % name, [hello, frame(TEXT, b"x", rsv=bit), frame(PING)], [0, 1, 0])
        row("3 %s allowed" % name, [frame(TEXT, b"x", rsv=bit), frame(PING, rsv=bit)], [0, 0], rsv=bit)
        row("3 %s with another one allowed" % name, [frame(BIN, b"x", rsv=bit)], [1], rsv=0x70 & ~bit)
    row("3 all RSV, all allowed", [frame(TEXT, b"x", rsv=0x70)], [0], rsv=0x70)
    row("3 RSV on a close", [close(1000, rsv=0x40), frame(PING)], [1, A])
    # 4: reserved opcodes (with FIN: nothing else is wrong with them)
    for op in (3, 4, 5, 6, 7, 11, 12, 13, 14, 15):
        row("4 opcode %d" % op, [hello, frame(op, b"z"), frame(PING)], [0, 2, 0])
    row("4 opcode 3 without FIN opens a message: frames in error count", [frame(3, b"z", fin=0), frame(CONT, b"y")], [2, 0])
    # 5: fragmentation
    row("5.3 text in two", [frame(TEXT, b"a", fin=0), frame(CONT, b"b")], [0, 0])
    row("5.6 ping between fragments", [frame(TEXT, b"a", fin=0), frame(PING, b"p"), frame(CONT, b"b", fin=0),
                                       frame(PONG), frame(CONT)], [0, 0, 0, 0, 0])
    row("5.9 continuation first", [frame(CONT, b"a"), hello], [8, 0])
    row("5.10 continuation first, no FIN", [frame(CONT, b"a", fin=0), frame(CONT, b"b")], [8, 0])
    row("5.15 continuation after a message", [hello, frame(CONT, b"a", fin=0), frame(CONT)], [0, 8, 0])
    row("5.x text inside an open text", [frame(TEXT, b"a", fin=0), frame(TEXT, b"b"), frame(CONT, b"c")], [0, 9, 8])
    row("5.x binary inside an open text, no FIN", [frame(TEXT, b"a", fin=0), frame(BIN, b"b", fin=0), frame(CONT)],
        [0, 9, 0])
    # 7: close
    row("7.1 close empty", [hello, close()], [0, 0])
    row("7.3.2 close length 1", [close(reason=b"a")], [6])
    row("7.3.3 close length 2", [close(1000)], [0])
    row("7.3.4 close with reason", [close(1000, b"bye")], [0])
    row("7.3.6 close 126", [close(1000, b"r" * 124)], [5])
    row("7.1.x frames after close", [close(1000), hello, frame(PING), close(999), frame(3)], [0, A, A, A, A])
    row("7.x close inside an open message", [frame(TEXT, b"a", fin=0), close(1001), frame(CONT)], [0, 0, A])
    row("7.x close without FIN", [close(1000, fin=0)], [4])
    for code, ok in ((999, 0), (1000, 1), (1004, 0), (1005, 0), (1006, 0), (1011, 1), (1014, 1), (1015, 0), (2999, 0),
                     (3000, 1), (4999, 1), (5000, 0), (0, 0), (1003, 1), (1007, 1), (1016, 0), (65535, 0)):
        row("7.9 close %d" % code, [hello, close(code)], [0, 0 if ok else 7])
    # masking
    row("5.1 unmasked under EXPECT_MASKED", [hello, frame(TEXT, b"x", masked=False)], [0, 3])
    row("5.1 masked under EXPECT_UNMASKED", [frame(TEXT, b"x", masked=False), hello], [0, 3], flags=EU)
    row("5.1 either without an EXPECT flag", [frame(TEXT, b"x", masked=False), hello], [0, 0], flags=0)
    row("order: RSV before opcode before mask", [frame(5, b"x", rsv=0x20, masked=False), frame(5, masked=False)], [1, 2])
    return t


# ---------------------------------------------------------------------------------------------
# scripts of many frames

def quiet(n, tail_open=False):
    """n valid frames: one-byte messages of one or two fragments and a ping now and then; the
    last one leaves its message open when tail_open"""
    out = []
    while len(out) < n:
        left = n - len(out)
        if len(out) % 7 == 3:
            out.append(frame(PING, b"p"))
        elif left >= 2 and len(out) % 3 == 0:
            out += [frame(TEXT, b"a", fin=0), frame(CONT, b"b")]
        else:
            out.append(frame(BIN, b"c"))
    if tail_open and out:
        out[-1] = frame(TEXT, b"a", fin=0) if out[-1][0] & 15 != CONT else frame(CONT, b"b", fin=0)
    return out


def carry_script():
    """nine frames of one connection: an open message with a ping in the middle that a limit of 6
    bytes stops at its fifth frame (7 bytes), a message, a message left open, a close, a frame
    after the close"""
    return [frame(TEXT, b"ab", fin=0), frame(CONT, b"c", fin=0), frame(PING, b"p"), frame(CONT, b"de", fin=0),
            frame(CONT, b"fg"), frame(BIN, b"x"), frame(TEXT, b"h", fin=0), close(1000), frame(PING)]


def error_frame(kind, is_open, limit, nbytes=0, masked=True):
    """a frame whose code is `kind` on a connection with the given open / bytes state (every
    kind is built so that no earlier rule fails; 3 needs the EXPECT flag that `masked` obeys, 10 a
    limit)"""
    def fr(*a, **kw):
        return frame(*a, masked=masked, **kw)
    if kind == 1:
        return fr(PING, rsv=0x20)
    if kind == 2:
        return fr(11, b"z")
    if kind == 3:
        return frame(PONG, b"u", masked=not masked)
    if kind == 4:
        return fr(PING, b"f", fin=0)
    if kind == 5:
        return fr(PONG, b"l" * 126)
    if kind == 6:
        return fr(CLOSE, b"x")
    if kind == 7:
        return fr(CLOSE, (1005).to_bytes(2, "big"))
    if kind == 8:
        assert not is_open
        return fr(CONT, b"c")
    if kind == 9:
        assert is_open
        return fr(TEXT, b"t")
    assert kind == 10 and limit
    body = b"B" * (max(0, limit - nbytes) + 1)
    return fr(CONT, body) if is_open else fr(BIN, body)


PLAIN = (1, 2, 3, 4, 5, 8, 9, 10)                         # the kinds that leave the connection open


class Model:
    """the generator's own track of open / bytes (to aim an error; never an expected value)"""

    def __init__(self):
        self.open, self.bytes, self.closed = False, 0, False

    def push(self, f):
        op, fin = f[0] & 15, f[0] >> 7
        n = f[1] & 0x7F
        n = int.from_bytes(f[2:4], "big") if n == 126 else n
        if op == CLOSE:
            self.closed = True
        if not op & 8 and not self.closed:
            self.open, self.bytes = (False, 0) if fin else (True, self.bytes + n)
        return f


def random_segment(rng, n, flags, rsv_allowed, limit, err_rate, aimed=None, quiet_until=0):
    """n frames, mostly valid, masked unless the flags expect unmasked ones; each frame from index
    quiet_until on is an error of a random kind with probability err_rate; aimed: {k: kind} errors
    at chosen indices (the frame before is chosen to make 8 / 9 possible)"""
    m, out = Model(), []
    mk = not flags & P.EXPECT_UNMASKED

    def fr(*a, **kw):
        return frame(*a, masked=mk, **kw)
    kinds = [k for k in range(1, 11) if not (k == 3 and not flags & (P.EXPECT_MASKED | P.EXPECT_UNMASKED))
             and not (k == 10 and not 0 < limit < 16) and not (k == 1 and rsv_allowed & 0x20)]
    aimed = aimed or {}
    close_at = n - int(rng.integers(1, 4)) if rng.random() < 0.15 and not aimed else -1
    while len(out) < n:
        k = len(out)
        kind = aimed.get(k, int(rng.choice(kinds)) if k >= quiet_until and rng.random() < err_rate else 0)
        if kind not in kinds:
            kind = 0
        if kind in (6, 7) and k != close_at and k not in aimed and (aimed or k < n - 3):
            kind = 4 if kind == 6 else 5                      # a CLOSE in the middle would fence the rest off
        if kind == 8 and m.open:
            kind = 9
        elif kind == 9 and not m.open:
            kind = 8
        if not aimed and k >= n - 3 and k != close_at and rng.random() < 0.1:
            kind = 6 + int(rng.integers(0, 2))            # CLOSE errors near a segment's end
        want = aimed.get(k + 1)
        if want in (1, 2, 3, 4, 5):                           # a control frame: the one after it sees the same state
            want = aimed.get(k + 2)
        if kind:
            f = error_frame(kind, m.open, limit, m.bytes, mk)
        elif k == close_at:
            f = fr(CLOSE, int(rng.choice([1000, 1001, 3000, 4999])).to_bytes(2, "big") + b"r" * int(rng.integers(0, 2))) \
                if rng.random() < 0.7 else fr(CLOSE)
        elif want in (8, 9) and m.open != (want == 9):
            f = fr(TEXT, b"o", fin=0) if want == 9 else fr(CONT, b"e")
        elif m.open:
            r = rng.random()
            room = limit == 0 or m.bytes + 1 <= limit
            f = fr(PING if r < 0.5 else PONG, b"p" * int(rng.integers(0, 4))) if r < 0.2 else \
                fr(CONT, b"c" if room else b"", fin=int(r < 0.7))
        else:
            r = rng.random()
            nb = int(rng.integers(0, 4))
            nb = min(nb, limit) if limit else nb
            f = fr(PING if r < 0.1 else PONG, b"q" * int(rng.integers(0, 4))) if r < 0.2 else \
                fr(TEXT if r < 0.6 else BIN, b"d" * nb, fin=int(r < 0.75), rsv=rsv_allowed & 0x40 if r > 0.9 else 0)
        out.append(m.push(f))
    return out


def list_starts(batch):
    """where each segment's frame 0 stands in the list of all counted frames of the batch, laid
    end to end in segment order: the check's kernels cut that list into tiles of 256"""
    n = np.minimum(batch.res["n_frames"].astype(np.int64), batch.max_frames)
    return np.concatenate([[0], np.cumsum(n)[:-1]])


def random_cases(seed=2011):
    """The seeded random cases of the GPU suite: [(batch, flags, rsv_allowed, limit, state in)].
    1000 segments of 1..40 frames in ten batches of 100, and 8 segments of 200..1100 frames in
    batches of their own (so their frame k stands at list position k). Tiles are cut from the list
    of all frames of a batch (list_starts): the long segments' errors are aimed at the last and
    first frame of every tile; in the short batches every segment that crosses a tile edge takes
    one error there, before or after the edge in turn, with no other error before it, so that it
    is the segment's first_bad; one segment in eight of the others has its only error on its last
    frame. Flags, rsv_allowed and the limit are drawn per batch; one segment in
    twelve ends in a frame that is counted but not consumed; one in eight starts from a carried
    state."""
    rng = np.random.default_rng(seed)
    cases = []
    aim = [0, 0, 0, 0, 0, 0]
    for b in range(18):
        long_ = b >= 10
        flags = (P.EXPECT_MASKED, P.EXPECT_MASKED, P.EXPECT_MASKED, P.EXPECT_UNMASKED, 0)[b % 5] | \
            (P.WIRE_MASKED if rng.random() < 0.5 else 0)
        rsv_allowed = int(rng.choice([0, 0x40, 0x70]))
        limit = int(rng.choice([3, 7] if long_ else [0, 3, 7, 1 << 40]))
        segs, start = [], 0
        for s in range(1 if long_ else 100):
            n = int(rng.integers(200, 1101)) if long_ else int(rng.integers(1, 41))
            aimed, quiet_until = {}, 0
            if long_ and n > 257:
                edges = list(range(255, n - 1, 256))
                for k in edges[:-1]:
                    aimed[k] = PLAIN[aim[0] % 8]
                    aimed[k + 1] = PLAIN[(aim[1] * 3 + 1) % 8]
                    aim[0] += 1
                    aim[1] += 1
                # the last tile edge takes the CLOSE errors, which fence the rest of the segment off
                k, odd = edges[-1], (b - 10) % 2
                aimed[k + odd] = 6 + (aim[2] // 2) % 2
                if odd:
                    aimed[k] = PLAIN[aim[0] % 8]
                    aim[0] += 1
                aim[2] += 1
            elif not long_:
                k = 255 - start % 256                         # the segment's frame on a tile's last thread
                if k + 1 < n and aim[3] % 2 == 0:
                    aimed[k] = 1 + (aim[3] // 2) % 10
                elif k + 1 < n:
                    aimed[k + 1] = 1 + (aim[4] * 3) % 10
                    aim[4] += 1
                if k + 1 < n:
                    aim[3] += 1
                    quiet_until = n
                elif rng.random() < 0.12:                     # one error, on the segment's last frame
                    aimed[n - 1] = 1 + aim[5] % 10
                    aim[5] += 1
                    quiet_until = n
            segs.append(random_segment(rng, n, flags, rsv_allowed, limit, 0.01 if long_ else 0.08, aimed, quiet_until))
            start += n
        mf = max(len(f) for f in segs) + int(rng.integers(0, 3))
        batch = Batch(segs, mf, gap=int(rng.integers(0, 5)))
        state = np.zeros(batch.nseg, np.uint64)
        for s in range(batch.nseg):
            if rng.random() < 1 / 12:
                batch.unconsume_last(s, -4 if rng.random() < 0.5 else -1)
            if rng.random() < 1 / 8 and not long_:
                state[s] = int(rng.choice([P.ST_OPEN | 2, P.ST_OPEN | 7, P.ST_CLOSED, P.ST_OPEN]))
        cases.append((batch, flags, rsv_allowed, limit, state))
    return cases


CLASSES = {"first", "interior", "tile_last", "tile_first", "last"}


def classes(k, n, pos):
    """position classes of frame k of n at list position pos: a tile's last frame stands at
    pos % 256 == 255, its first at pos % 256 == 0 (with k > 0: a frame that has frames of its own
    segment in the tile before)"""
    out = set()
    if k == 0:
        out.add("first")
    if k == n - 1:
        out.add("last")
    if pos % 256 == 255:
        out.add("tile_last")
    if k and pos % 256 == 0:
        out.add("tile_first")
    if pos % 256 not in (0, 255) and k not in (0, n - 1):
        out.add("interior")
    return out


def coverage(cases):
    """(first_bad count per code, {code: position classes its frames show in}, {code: position
    classes it shows in as a segment's first_bad}, AFTER_CLOSE count, NOT_CONSUMED count) of the
    oracle's answers over the cases; positions are list positions (list_starts)"""
    first = {c: 0 for c in range(1, 11)}
    where = {c: set() for c in range(1, 11)}
    where_first = {c: set() for c in range(1, 11)}
    after = notc = 0
    for batch, flags, rsv_allowed, limit, state in cases:
        codes, res, _ = batch.expect(flags, rsv_allowed, limit, state)
        starts = list_starts(batch)
        for s in range(batch.nseg):
            n = int(batch.res[s]["n_frames"])
            if res[s]["first_bad"] != P.NONE:
                k = int(res[s]["first_bad"])
                first[int(res[s]["code"])] += 1
                where_first[int(res[s]["code"])] |= classes(k, n, int(starts[s]) + k)
            row = codes[s * batch.max_frames:s * batch.max_frames + n]
            after += int((row == P.AFTER_CLOSE).sum())
            notc += int((row == P.NOT_CONSUMED).sum())
            for k in np.nonzero((row >= 1) & (row <= 10))[0]:
                where[int(row[k])] |= classes(int(k), n, int(starts[s]) + int(k))
    return first, where, where_first, after, notc
