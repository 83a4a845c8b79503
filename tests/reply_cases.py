"""Builders of the control replies' test cases (tests/test_reply_host.py on the CPU,
tests/test_gpu_reply.py on the GPU): the directed table with its reply bytes written by hand, and
the seeded random batches with their coverage count. Frames and batches are proto_cases.py's.
Expected values never come from here: they are the table's literals or reply_oracle.replies()."""
import numpy as np

import proto_cases as PC
import proto_oracle as P
import reply_oracle as R
from proto_cases import BIN, CLOSE, CONT, PING, PONG, TEXT, close, frame

N = R.NONE
K1 = 0x3D21FA37                                           # RFC 6455 5.7's example key 37 FA 21 3D as a u32, low byte first
K2 = 0x04030201                                           # 01 02 03 04
LAST = R.LAST_PING_ONLY


def x(body, kb):
    return bytes(b ^ kb[i & 3] for i, b in enumerate(body))


KB1, KB2 = bytes([0x37, 0xFA, 0x21, 0x3D]), bytes([1, 2, 3, 4])


def directed_table():
    """rows: dict(name, frames, flags (without WIRE_MASKED: the feeder decides), proto (first_bad,
    close_status) or None, fail, keyed (every PONG slot holds K1, the CLOSE slot K2), state (None:
    no carry), unconsume (the last frame is counted but not consumed), tx (the reply, by hand),
    res (n_pong, close_kind, close_status, tx_len), state_out)"""
    t = []

    def row(name, frames, tx, res, flags=0, proto=None, fail=0, keyed=False, state=0, state_out=None, unconsume=False):
        sent = R.ST_CLOSE_SENT if res[1] else 0
        t.append(dict(name=name, frames=frames, flags=flags, proto=proto, fail=fail, keyed=keyed, state=state,
                      unconsume=unconsume, tx=tx, res=res + (len(tx),),
                      state_out=(None if state is None else state | sent) if state_out is None else state_out))

    hello = frame(TEXT, b"Hel")
    b125 = bytes(range(125))
    # 5.5.2, 5.5.3: pings
    row("ping empty", [frame(PING)], b"\x8a\x00", (1, 0, 0))
    row("ping hello", [frame(PING, b"hello")], b"\x8a\x05hello", (1, 0, 0))
    row("ping unmasked on the wire", [frame(PING, b"hi", masked=False)], b"\x8a\x02hi", (1, 0, 0))
    row("ping 125", [frame(PING, b125)], b"\x8a\x7d" + b125, (1, 0, 0))
    row("ping 126: not answered", [frame(PING, b"\xfe" * 126), hello], b"", (0, 0, 0))
    row("ping without FIN: not answered", [frame(PING, b"a", fin=0), frame(PING, b"b")], b"\x8a\x01b", (1, 0, 0))
    row("pings in order, data between", [frame(PING, b"1"), hello, frame(PING, b"22"), frame(PONG, b"x"), frame(PING)],
        b"\x8a\x011\x8a\x0222\x8a\x00", (3, 0, 0))
    row("only the most recent ping", [frame(PING, b"1"), hello, frame(PING, b"22"), frame(PING, b"333"), hello],
        b"\x8a\x03333", (1, 0, 0), flags=LAST)
    row("most recent: the 126-byte ping is not one", [frame(PING, b"1"), frame(PING, b"z" * 126)], b"\x8a\x011", (1, 0, 0),
        flags=LAST)
    row("unsolicited pong, data: silence", [frame(PONG, b"abc"), hello, frame(BIN, b"")], b"", (0, 0, 0))
    row("empty segment", [], b"", (0, 0, 0))
    row("ping counted but not consumed", [frame(PING, b"a"), frame(PING, b"b")], b"\x8a\x01a", (1, 0, 0), unconsume=True)
    # 5.5.1: the CLOSE echo
    row("close 1000", [close(1000)], b"\x88\x02\x03\xe8", (0, 1, 1000))
    row("close empty", [hello, close()], b"\x88\x00", (0, 1, 0))
    row("close of one byte: empty echo", [close(reason=b"a")], b"\x88\x00", (0, 1, 0))
    row("close with reason: the reason is not echoed", [close(1001, b"going away")], b"\x88\x02\x03\xe9", (0, 1, 1001))
    row("close 125", [close(3000, b"r" * 123)], b"\x88\x02\x0b\xb8", (0, 1, 3000))
    row("close unmasked on the wire", [close(4999, masked=False)], b"\x88\x02\x13\x87", (0, 1, 4999))
    row("ping, close, ping: nothing after the close", [frame(PING, b"a"), close(1000), frame(PING, b"b"), close(1001)],
        b"\x8a\x01a\x88\x02\x03\xe8", (1, 1, 1000))
    row("most recent ping before the close", [frame(PING, b"a"), frame(PING, b"b"), close(), frame(PING, b"c")],
        b"\x8a\x01b\x88\x00", (1, 1, 0), flags=LAST)
    row("close counted but not consumed", [frame(PING, b"a"), close(1000)], b"\x8a\x01a", (1, 0, 0), unconsume=True)
    # 7.1.7: the protocol check's status
    row("first_bad after a ping", [frame(PING, b"a"), frame(TEXT, b"x", rsv=0x40), frame(PING, b"b")],
        b"\x8a\x01a\x88\x02\x03\xea", (1, 2, 1002), proto=(1, 1002))
    row("first_bad on frame 0, a ping", [frame(PING, b"a", rsv=0x10), frame(PING, b"b")], b"\x88\x02\x03\xea", (0, 2, 1002),
        proto=(0, 1002))
    row("too big: 1009", [hello, frame(PING), frame(BIN, b"B" * 9)], b"\x8a\x00\x88\x02\x03\xf1", (1, 2, 1009),
        proto=(2, 1009))
    row("first_bad before the close", [frame(CONT, b"a"), frame(PING, b"p"), close(1000)], b"\x88\x02\x03\xea", (0, 2, 1002),
        proto=(0, 1002))
    row("first_bad is the close", [frame(PING, b"p"), close(1005)], b"\x8a\x01p\x88\x02\x03\xea", (1, 2, 1002),
        proto=(1, 1002))
    row("first_bad after the close: echo", [close(1000), frame(PING, b"p")], b"\x88\x02\x03\xe8", (0, 1, 1000),
        proto=(1, 1002))
    row("no error", [frame(PING, b"p")], b"\x8a\x01p", (1, 0, 0), proto=(N, 0))
    row("most recent ping before first_bad", [frame(PING, b"a"), frame(PING, b"b"), frame(7), frame(PING, b"c")],
        b"\x8a\x01b\x88\x02\x03\xea", (1, 2, 1002), flags=LAST, proto=(2, 1002))
    row("protocol wins over the caller", [frame(7)], b"\x88\x02\x03\xea", (0, 2, 1002), proto=(0, 1002), fail=1007)
    # the caller's status
    row("caller 1007", [hello, frame(PING, b"p")], b"\x8a\x01p\x88\x02\x03\xef", (1, 3, 1007), fail=1007)
    row("caller 1001 wins over the echo", [frame(PING, b"p"), close(1000), frame(PING)], b"\x8a\x01p\x88\x02\x03\xe9",
        (1, 3, 1001), fail=1001)
    row("caller: the low 16 bits", [], b"\x88\x02\x03\xf3", (0, 3, 1011), fail=0x7001_03F3)
    row("caller: low 16 bits zero", [], b"\x88\x02\x00\x00", (0, 3, 0), fail=0x10000)
    # the carry
    row("close already sent", [frame(PING, b"a"), close(1000)], b"", (0, 0, 0), state=R.ST_CLOSE_SENT, fail=1001,
        proto=(0, 1002))
    row("no state", [frame(PING, b"a"), close(1000)], b"\x8a\x01a\x88\x02\x03\xe8", (1, 1, 1000), state=None)
    # client role
    row("client: masked pong", [frame(PING, b"ab", masked=False)], b"\x8a\x82" + KB1 + x(b"ab", KB1), (1, 0, 0), keyed=True)
    row("client: masked pong 125 and echo", [frame(PING, b125, masked=False), close(1000, masked=False)],
        b"\x8a\xfd" + KB1 + x(b125, KB1) + b"\x88\x82" + KB2 + x(b"\x03\xe8", KB2), (1, 1, 1000), keyed=True)
    row("client: empty pong, empty close", [frame(PING), close()], b"\x8a\x80" + KB1 + b"\x88\x80" + KB2, (1, 1, 0),
        keyed=True)
    row("client: caller 1001", [], b"\x88\x82" + KB2 + x(b"\x03\xe9", KB2), (0, 3, 1001), keyed=True, fail=1001)
    return t


class Case:
    """A proto_cases.Batch with the reply call's per-segment inputs; expect() is the model's answer
    for the wire the flags name (still masked under WIRE_MASKED, else as the in-place decode leaves it)"""

    def __init__(self, batch, flags=0, proto=None, fail=None, keys=None, state=None):
        self.b, self.flags, self.fail, self.keys, self.state = batch, flags, fail, keys, state
        self.proto = None
        if proto is not None:                                   # [(first_bad, close_status)] per segment
            self.proto = np.zeros(batch.nseg, P.RES_DTYPE)
            self.proto["close_frame"] = N
            for s, (fb, st) in enumerate(proto):
                self.proto[s]["first_bad"], self.proto[s]["close_status"] = fb, st
                self.proto[s]["code"] = 0 if fb == N else (10 if st == 1009 else 2)

    def wire(self, flags=None):
        return self.b.raw if (self.flags if flags is None else flags) & R.WIRE_MASKED else self.b.dec

    def expect(self, flags=None, state="own"):
        flags = self.flags if flags is None else flags
        return R.replies(self.wire(flags), self.b.seg_off, self.b.desc, self.b.res, self.b.max_frames, flags, self.proto,
                         self.fail, self.keys, self.state if isinstance(state, str) else state)


def table_case(rows, wire_masked=0, gap=3):
    """rows of the directed table that share flags, keyed and "has a state" as one batch, one
    connection per segment"""
    mf = max(len(r["frames"]) for r in rows) + 1
    b = PC.Batch([r["frames"] for r in rows], mf, gap=gap)
    for s, r in enumerate(rows):
        if r["unconsume"]:
            b.unconsume_last(s, -4)
    keys = None
    if rows[0]["keyed"]:
        keys = np.full(b.nseg * (mf + 1), K1, np.uint32)
        keys[mf::mf + 1] = K2
    state = None if rows[0]["state"] is None else np.array([r["state"] for r in rows], np.uint32)
    return Case(b, rows[0]["flags"] | wire_masked, [r["proto"] or (N, 0) for r in rows],
                np.array([r["fail"] for r in rows], np.uint32), keys, state)


def table_groups():
    groups = {}
    for r in directed_table():
        groups.setdefault((r["flags"], r["keyed"], r["state"] is None), []).append(r)
    return list(groups.values())


def table_expect(rows):
    """(tx, tx_off, result records, state out) from the rows' literals"""
    tx = b"".join(r["tx"] for r in rows)
    off = np.concatenate([[0], np.cumsum([len(r["tx"]) for r in rows])]).astype(np.uint64)
    res = np.array([r["res"] for r in rows], np.uint32).view(R.RES_DTYPE).reshape(-1)
    st = None if rows[0]["state"] is None else np.array([r["state_out"] for r in rows], np.uint32)
    return tx, off, res, st


# ---------------------------------------------------------------------------------------------
# seeded random batches

def random_segment(rng, n, masked):
    """n frames: data, pings of every kind (answerable, too long, without FIN), pongs, and a CLOSE
    one time in three somewhere in the last third"""
    out = []
    close_at = int(rng.integers(n - n // 3 - 1, n)) if n and rng.random() < 0.33 else -1
    for k in range(n):
        r = rng.random()
        if k == close_at:
            body = b"" if r < 0.2 else (b"x" if r < 0.3 else int(rng.choice([1000, 1001, 3000, 0x3412])).to_bytes(2, "big") +
                                        b"r" * int(rng.integers(0, 4)))
            out.append(frame(CLOSE, body, masked=masked))
        elif r < 0.35:
            ln = int(rng.choice([0, 1, 2, 3, 4, 5, 16, 17, 124, 125, 126]))
            out.append(frame(PING, bytes(rng.integers(0, 256, ln, dtype=np.uint8)), fin=int(rng.random() > 0.1), masked=masked))
        elif r < 0.45:
            out.append(frame(PONG, b"q" * int(rng.integers(0, 4)), masked=masked))
        else:
            out.append(frame(BIN if r < 0.8 else TEXT, b"d" * int(rng.integers(0, 9)), masked=masked))
    return out


def random_cases(seed=6455, nbatch=12, nseg=40):
    """[Case]: batches of nseg segments of 0..24 frames (one segment in ten empty). Drawn per batch:
    WIRE_MASKED, LAST_PING_ONLY, the role (keys or none), a state array or none; per segment: a
    first_bad (one in four, before, at or after its CLOSE), a fail status (one in five), a carried
    CLOSE_SENT (one in six), a last frame that is not consumed (one in ten)."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(nbatch):
        flags = (R.WIRE_MASKED if i & 1 else 0) | (LAST if i & 2 else 0)
        keyed, stated = bool(i & 4), i % 3 != 2
        segs = [random_segment(rng, 0 if rng.random() < 0.1 else int(rng.integers(1, 25)), masked=not keyed or rng.random() < 0.5)
                for _ in range(nseg)]
        mf = max(len(f) for f in segs) + int(rng.integers(0, 3))
        b = PC.Batch(segs, mf, gap=int(rng.integers(0, 5)))
        proto, fail = [], np.zeros(nseg, np.uint32)
        state = np.zeros(nseg, np.uint32) if stated else None
        for s, fr in enumerate(segs):
            if fr and rng.random() < 0.1:
                b.unconsume_last(s, -4)
            proto.append((int(rng.integers(0, len(fr))), int(rng.choice([1002, 1009]))) if fr and rng.random() < 0.25 else (N, 0))
            if rng.random() < 0.2:
                fail[s] = int(rng.choice([1001, 1007, 0x20000 | 1011]))
            if stated and rng.random() < 1 / 6:
                state[s] = R.ST_CLOSE_SENT
        keys = rng.integers(0, 1 << 32, nseg * (mf + 1), dtype=np.uint64).astype(np.uint32) if keyed else None
        cases.append(Case(b, flags, proto if i % 4 != 3 else None, fail if i % 5 != 4 else None, keys, state))
    return cases


def coverage(cases):
    """what the model's answers over the cases show"""
    seen = {"kinds": set(), "roles": set(), "wire_masked": set(), "last": set(), "empty": 0, "carried": 0, "pongs": 0,
            "silenced": 0}
    for c in cases:
        _tx, _off, res, _st = c.expect()
        seen["kinds"] |= set(int(k) for k in res["close_kind"])
        seen["roles"].add(c.keys is not None)
        seen["wire_masked"].add(bool(c.flags & R.WIRE_MASKED))
        seen["last"].add(bool(c.flags & LAST))
        seen["empty"] += int((c.b.res["n_frames"] == 0).sum())
        seen["pongs"] += int(res["n_pong"].sum())
        if c.state is not None:
            seen["carried"] += int((c.state & R.ST_CLOSE_SENT).astype(bool).sum())
            alone = c.expect(state=None)[2]
            seen["silenced"] += int(((c.state & R.ST_CLOSE_SENT) != 0)[alone["tx_len"] > 0].sum())
    return seen
