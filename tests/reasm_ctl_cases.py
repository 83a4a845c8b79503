"""Byte streams for the control-frame reassembly fixture (tests/golden/reassemble_ctl.json).

As tests/reasm_cases.py: each case is ONE connection's rx byte stream, rebuilt from a seed and
pinned by its SHA-256 in the fixture. The fixture's deliveries come from the reference's own
reactor stack with a glue that leaves pktype = 0 for control frames (tests/c/ctl_glue.c), the
rule of WEBSOCKET_REASM_CONTROL_DIRECT: a control frame (opcode 8-15) goes straight to on_recv,
past the fragment cache, whatever is pending and whatever its FIN bit.
"""
import numpy as np

from reasm_cases import frame, message, sha256  # noqa: F401

PING, PONG, CLOSE = 0x89, 0x8A, 0x88


def _fragments(rng, sizes, opcode=2, masked=True):
    """the frames of one fragmented message, as a list"""
    n = len(sizes)
    return [frame(rng, (opcode if k == 0 else 0) | (0x80 if k == n - 1 else 0), int(s), masked=masked)
            for k, s in enumerate(sizes)]


def _ping_between(rng):
    # a ping between the fragments of a message, at every gap of messages of 2..6 fragments
    parts = []
    for i in range(60):
        fr = _fragments(rng, [int(x) for x in rng.integers(0, 2000, int(rng.integers(2, 7)))], opcode=1 + i % 2)
        at = 1 + i % (len(fr) - 1)
        fr.insert(at, frame(rng, PING, int(rng.integers(0, 126))))
        parts += fr
    return b"".join(parts), 0


def _control_runs(rng):
    # several control frames in a row: at the stream's start, inside a message, between messages
    parts = [frame(rng, PING, 3), frame(rng, PONG, 0), frame(rng, CLOSE, 2)]
    for i in range(30):
        fr = _fragments(rng, [int(x) for x in rng.integers(0, 500, int(rng.integers(1, 5)))])
        run = [frame(rng, int(rng.choice([PING, PONG])), int(rng.integers(0, 126))) for _ in range(int(rng.integers(2, 6)))]
        at = int(rng.integers(0, len(fr) + 1))
        parts += fr[:at] + run + fr[at:]
    return b"".join(parts), 0


def _close_after_open(rng):
    # a message left open (no FIN fragment ever comes), then CLOSE: delivered, the message stays pending
    s = message(rng, [100, 200]) + b"".join(_fragments(rng, [700, 800, 900])[:2]) + frame(rng, CLOSE, 2)
    return s, 0


def _control_no_fin(rng):
    # control frames with FIN = 0 (not legal, and not looked at): still delivered directly, alone
    parts = []
    for i in range(20):
        fr = _fragments(rng, [int(x) for x in rng.integers(1, 300, 3)])
        fr.insert(1 + i % 2, frame(rng, 0x09 + i % 2, int(rng.integers(0, 126))))
        parts += fr
    parts.append(frame(rng, 0x08, 5))
    return b"".join(parts), 0


def _control_bodies(rng):
    # empty, unmasked, 125-byte and 70,000-byte control bodies (the codec does not enforce 125),
    # non-minimal length forms
    parts = []
    for i, (n, masked, form) in enumerate([(0, True, None), (0, False, None), (125, True, None), (125, False, 16),
                                           (70000, True, None), (1, True, 64), (126, False, None),
                                           (65536, False, None)]):
        fr = _fragments(rng, [300, 20000, 5], masked=bool(i % 2))
        fr.insert(1 + i % 2, frame(rng, PING if i % 2 else PONG, n, masked=masked, form=form))
        parts += fr
    return b"".join(parts), 0


def _opcodes(rng):
    # reserved control opcodes 0xB-0xF go direct as well; data opcodes 3-7 stay data (with
    # FIN they close the pending message, without they join it)
    parts = []
    for op in (0xB, 0xC, 0xD, 0xE, 0xF, 3, 4, 5, 6, 7):
        for fin in (0x80, 0):
            fr = _fragments(rng, [50, 60, 70])
            fr.insert(1, frame(rng, fin | op, int(rng.integers(0, 100))))
            parts += fr
    return b"".join(parts), 0


def _limit_control_uncounted(rng):
    # limit 1000: 400 cached, a 5000-byte ping (would overflow if it were counted), then a
    # 600-byte fragment that exactly fits; the next message's 400 + 601 does not
    s = (frame(rng, 0x02, 400) + frame(rng, PING, 5000) + frame(rng, 0x80, 600) +
         frame(rng, 0x02, 400) + frame(rng, PING, 10) + frame(rng, 0x80, 601) + message(rng, [5]))
    return s, 1000


def _limit_overflow_after_control(rng):
    # limit 5000, 1000-B fragments with a ping after each: the 6th fragment overflows right
    # after a control frame, which was delivered
    fr = []
    for f in _fragments(rng, [1000] * 7):
        fr += [f, frame(rng, PING, 100)]
    return message(rng, [1000] * 3) + b"".join(fr) + message(rng, [10, 10]), 5000


def _limit_boundary(rng):
    # limit 3000: 1000 + 1000 cached, a ping, + 1000 is exactly the limit (no overflow); then
    # 2001, a ping, + 1000 overflows
    s = (frame(rng, 0x02, 1000) + frame(rng, 0x00, 1000) + frame(rng, PING, 64) + frame(rng, 0x80, 1000) +
         frame(rng, 0x02, 2001) + frame(rng, PING, 64) + frame(rng, 0x80, 1000) + message(rng, [5]))
    return s, 3000


def _limit_fin_unchecked(rng):
    # limit 100: a FIN data frame with nothing pending skips the check whatever its size, with
    # a large ping before it (never checked either); 40 + ping + 40 fits, 60 + ping + 50 does not
    s = (frame(rng, PING, 3000) + frame(rng, 0x82, 5000) + frame(rng, 0x02, 40) + frame(rng, PING, 200) +
         frame(rng, 0x80, 40) + frame(rng, PONG, 101) + frame(rng, 0x81, 300) + frame(rng, 0x02, 60) +
         frame(rng, PING, 7) + frame(rng, 0x80, 50))
    return s, 100


def _tail(rng):
    # ends inside a control frame that follows an open fragment: the reactor keeps the tail
    s = b"".join(message(rng, [int(x) for x in rng.integers(0, 3000, int(rng.integers(1, 4)))]) for _ in range(10))
    s += frame(rng, 0x02, 300) + frame(rng, PING, 20) + frame(rng, PING, 120)[:60]
    return s, 0


CASES = {
    "ping_between": (_ping_between, 105),
    "control_runs": (_control_runs, 106),
    "close_after_open": (_close_after_open, 107),
    "control_no_fin": (_control_no_fin, 108),
    "control_bodies": (_control_bodies, 109),
    "opcodes": (_opcodes, 110),
    "limit_control_uncounted": (_limit_control_uncounted, 111),
    "limit_overflow_after_control": (_limit_overflow_after_control, 112),
    "limit_boundary": (_limit_boundary, 113),
    "limit_fin_unchecked": (_limit_fin_unchecked, 114),
    "tail": (_tail, 115),
}


def build(name):
    """(wire bytes as a uint8 array, readcache_max_size) of case `name`"""
    fn, seed = CASES[name]
    wire, limit = fn(np.random.default_rng(seed))
    return np.frombuffer(wire, dtype=np.uint8).copy(), limit
