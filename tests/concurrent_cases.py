"""Jobs for the concurrency and workspace-reuse tests (tests/test_concurrent_cases.py on the CPU,
tests/test_gpu_concurrent_calls.py on the GPU). A job is one call of one device entry point: its
inputs, its output buffers filled with sentinels, and the outputs the suite's models expect, as
plain numpy. Nothing here is a new model: the expectations come from send_oracle, reply_oracle,
proto_oracle, text_oracle, client_oracle, the handshake fixture and host symbols, oracle_lib's
reassembly composition and enc_cases.encode_ref.

jobs(kind, n): n jobs of pairwise different (nseg, max_frames), so no two share a workspace
layout: a directed-table batch first, then shapes whose slot count nseg * max_frames lies just past
256 and 512, a batch of about 1000 segments of mixed lengths, and two more. hostile(kind): larger
batches of the same kind whose leftovers in the workspace are the worst a later, smaller call could
read. small(kind): two directed-size jobs of different layouts whose parts overlay a hostile
predecessor's non-zero parts (fewer segments with a larger max_frames, and the other way round)."""
import functools
import json
import os

import numpy as np

import client_cases as CC
import client_oracle as CO
import enc_cases as EC
import handshake_cases as HC
import proto_cases as PC
import proto_oracle as P
import reasm_cases as RS
import reply_cases as RC
import reply_oracle as R
import send_cases as SC
import send_oracle as S
import text_oracle as T
from oracle_lib import oracle_reassemble
from util_amd import wsframe as W

HERE = os.path.dirname(os.path.abspath(__file__))
FILL = 0xEE
NONE64 = 0xEEEEEEEEEEEEEEEE
TAIL = 64                         # sentinel bytes kept behind every output
MAX_SLOTS, MAX_WIRE = 70000, 8 << 20
WS_KINDS = ("text", "proto", "reply", "send")              # the kinds with a per-stream workspace of their own
KINDS = ("reasm", "encode", "text", "proto", "reply", "send", "sendlist", "handshake", "client_request", "client_verify")


def u8(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


def out_buf(expect, fill=FILL, tail=TAIL, mask=None):
    """(initial bytes, expected bytes, compared bytes or None) of an output: `expect` (any dtype) is
    what the call must leave, its untouched parts already holding `fill`; `tail` more fill bytes
    follow and must survive"""
    e = np.concatenate([u8(expect), np.full(tail, fill, np.uint8)])
    m = None if mask is None else np.concatenate([u8(mask).astype(bool), np.ones(tail, bool)])
    return np.full(len(e), fill, np.uint8), e, m


class Job:
    """ins: {name: numpy array or None}; par: scalars of the call; outs: {name: (initial bytes,
    expected bytes, mask of the compared bytes or None: all)}. An in/out array (a state word)
    starts from `initial` instead of the fill."""

    def __init__(self, kind, name, nseg, mf, ins, par, outs, wire_bytes=0):
        self.kind, self.name, self.nseg, self.mf = kind, name, nseg, mf
        self.ins, self.par, self.outs, self.wire_bytes = ins, par, outs, wire_bytes

    @property
    def shape(self):
        return self.nseg, self.mf

    @property
    def slots(self):
        return self.nseg * self.mf


def inout(words, fill=FILL):
    """an in/out state array: starts from `words[0]`, must end as `words[1]`, a sentinel behind it"""
    init, e, m = out_buf(words[1], fill)
    init[:len(u8(words[0]))] = u8(words[0])
    return init, e, m


# ------------------------------------------------------------------------------------------ send

@functools.lru_cache(maxsize=None)
def source():
    return SC.source()


def send_job(name, conns, frags, role, mm=None, exp=None, keys=None):
    src = source()
    msg, nmsg, mm = S.pack(conns, mm)
    if keys is None:
        keys = SC.keys_for(dict(role=role, conns=conns), mm)
    etx, eoff, emoff, eres = exp or S.batch(src, conns, frags, keys, mm)
    ins = dict(src=src, msg=msg, nmsg=nmsg, frags=np.asarray(frags, np.uint32), keys=keys)
    outs = dict(tx=out_buf(etx, tail=4096), tx_off=out_buf(eoff), moff=out_buf(emoff), res=out_buf(eres))
    return Job("send", name, len(conns), mm, ins, dict(cap=len(etx), role=role), outs, len(etx))


def send_mixed(nseg, mm, seed, role):
    """connections of 0..mm messages of mixed lengths, SKIP entries and range errors among them"""
    rng = np.random.default_rng(seed)
    conns, frags = [], []
    for _ in range(nseg):
        c = []
        for _ in range(int(rng.integers(0, mm + 1))):
            L = int(rng.choice([0, 1, 16, 125, 126, int(rng.integers(0, 600))]))
            kind = int(rng.integers(0, 30))
            so = int(rng.integers(0, SC.SRC_LEN - L))
            c.append((so, L, S.SKIP) if kind == 0 else ((SC.SRC_LEN, L + 1, 2) if kind == 1 else (so, L, 1 + kind % 2)))
        conns.append(c)
        frags.append(int(rng.choice([S.FRAG_DEFAULT, 2, 3, 50, 130, 1464]) + (4 if role else 0)) & 0xFFFFFFFF)
    return send_job("mixed %d x %d, role %d" % (nseg, mm, role), conns, frags, role, mm)


def send_tiled(name, period, pfrags, role, mm, nseg):
    """nseg connections: the connections of `period` again and again. The model runs on one period;
    its per-connection answers are repeated and the offsets are the running sum of the repeated
    lengths, which is exact: a connection stands alone (as tests/test_gpu_send.py does)."""
    src = source()
    pn = len(period)
    reps = -(-nseg // pn)
    tile = lambda a, per=1: np.tile(a, reps)[:nseg * per]  # noqa: E731
    pkeys = SC.keys_for(dict(role=role, conns=period), mm)
    ptx, poff, pmoff, pres = S.batch(src, period, pfrags, pkeys, mm)
    off = np.concatenate([[0], np.cumsum(tile(np.diff(poff.astype(np.int64))))]).astype(np.uint64)
    moff = tile(pmoff - np.repeat(poff[:-1], mm), mm) + np.repeat(off[:-1], mm)
    moff[tile(pmoff, mm) == NONE64] = NONE64
    tx = np.concatenate([np.tile(ptx, nseg // pn), ptx[:int(poff[nseg % pn])]])
    return send_job(name, (period * reps)[:nseg], tile(np.asarray(pfrags, np.uint32)), role, mm, exp=(tx, off, moff, tile(pres)),
                    keys=None if pkeys is None else tile(pkeys, mm))


def send_jobs():
    t = SC.list_rows()
    return [send_job(t[0]["name"], t[0]["conns"], t[0]["frags"], False), send_mixed(43, 6, 1, True), send_mixed(57, 9, 2, False),
            send_mixed(1000, 7, 3, True), send_job(t[3]["name"], t[3]["conns"][:13], t[3]["frags"][:13], True),
            send_mixed(300, 3, 4, False)]


def send_hostile():
    """every slot live, shard 1 (F = 3 in the server role, 7 in the client role: the smallest sizes
    that carry a byte), every message as long as the wire cap allows: records, piece pointers and
    loc[] dense and large. Then, F = 2 / 6 as the literal reading has it: too small to carry a byte,
    so every connection fails at message 0 and the summaries hold the smallest first_bad."""
    out = []
    for role, F in ((False, 3), (True, 7)):
        nseg, mm = 520, 12
        L = (MAX_WIRE // 2) // (nseg * mm * F)
        conn = [(17 + 5 * i, L - i, 1 + i % 2) for i in range(mm)]
        out.append(send_tiled("dense, F = %d" % F, [conn], [F], role, mm, nseg))
        out.append(send_tiled("F = %d carries nothing" % (F - 1), [conn], [F - 1], role, mm, nseg))
    return out


def send_small():
    t = SC.list_rows()
    a = send_job("small, 6 x 16", t[1]["conns"][8:14], t[1]["frags"][8:14], False)
    b = send_job("small, 16 x 3", [c[:3] for c in t[2]["conns"]], t[2]["frags"], True, 3)
    return [a, b]


# ----------------------------------------------------------------------------------------- reply

def reply_job(name, c, expect=None):
    b = c.b
    etx, eoff, eres, est = expect or c.expect()
    ins = dict(buf=c.wire(), seg_off=np.asarray(b.seg_off, np.uint64), desc=b.desc, res=b.res, proto=c.proto, fail=c.fail,
               keys=c.keys)
    outs = dict(tx=out_buf(np.frombuffer(etx, np.uint8)), tx_off=out_buf(eoff), rres=out_buf(eres))
    if c.state is not None:
        outs["state"] = inout((c.state, est))
    return Job("reply", name, b.nseg, b.max_frames, ins, dict(flags=c.flags, cap=len(etx), keyed=c.keys is not None), outs, len(etx))


def reply_mixed(nseg, mf, seed, keyed, stated=True):
    rng = np.random.default_rng(seed)
    segs = [RC.random_segment(rng, 0 if rng.random() < 0.1 else int(rng.integers(1, mf + 1)), masked=True) for _ in range(nseg)]
    b = PC.Batch(segs, mf, gap=int(rng.integers(0, 5)))
    proto = [(int(rng.integers(0, len(f))), int(rng.choice([1002, 1009]))) if f and rng.random() < 0.25 else (R.NONE, 0) for f in segs]
    fail = np.where(rng.random(nseg) < 0.2, 1001, 0).astype(np.uint32)
    state = np.where(rng.random(nseg) < 1 / 6, R.ST_CLOSE_SENT, 0).astype(np.uint32) if stated else None
    keys = rng.integers(0, 1 << 32, nseg * (mf + 1), dtype=np.uint64).astype(np.uint32) if keyed else None
    return reply_job("mixed %d x %d keyed %d" % (nseg, mf, keyed), RC.Case(b, R.LAST_PING_ONLY if seed & 1 else 0, proto, fail, keys, state))


def table_reply(keyed):
    rows = next(g for g in RC.table_groups() if g[0]["keyed"] == keyed and g[0]["flags"] == 0 and g[0]["state"] is not None)
    return reply_job("table keyed %d" % keyed, RC.table_case(rows), RC.table_expect(rows))


def reply_jobs():
    return [table_reply(False), reply_mixed(43, 6, 10, True), reply_mixed(57, 9, 11, False), reply_mixed(1000, 24, 12, True),
            table_reply(True), reply_mixed(300, 3, 13, False, stated=False)]


def reply_hostile():
    """every slot a PING with a 125-byte body and, last in its segment, a CLOSE: the records, the
    offsets and the counts as large as frames allow; unkeyed and keyed"""
    out = []
    for keyed in (False, True):
        nseg, mf = 260, 40
        period = [[PC.frame(PC.PING, bytes([65 + (s + k) % 26]) * 125) for k in range(mf - 1)] + [PC.close(1000 + s)] for s in range(4)]
        pb = PC.Batch(period, mf, gap=2)
        b = PC.Tiled(pb, nseg)
        pkeys = np.random.default_rng(5).integers(0, 1 << 32, 4 * (mf + 1), dtype=np.uint64).astype(np.uint32) if keyed else None
        tx, off, res, st = RC.Case(pb, 0, None, None, pkeys, np.zeros(4, np.uint32)).expect()
        exp = (tx * (nseg // 4), np.concatenate([[0], np.cumsum(b.tile(np.diff(off)))]).astype(np.uint64), b.tile(res), b.tile(st))
        c = RC.Case(b, 0, None, None, None if pkeys is None else b.tile(pkeys, mf + 1), np.zeros(nseg, np.uint32))
        out.append(reply_job("pings of 125 and a close, keyed %d" % keyed, c, exp))
    return out


def reply_small():
    return [reply_mixed(7, 60, 20, False), reply_mixed(45, 4, 21, True)]


# ----------------------------------------------------------------------------------------- proto

def proto_job(name, b, flags=P.EXPECT_MASKED, rsv=0, limit=0, state=None, expect=None):
    ecodes, eres, ewords = expect or b.expect(flags, rsv, limit, state)
    wire = b.raw if flags & P.WIRE_MASKED else b.dec
    ins = dict(buf=wire, seg_off=np.asarray(b.seg_off, np.uint64), desc=b.desc, res=b.res)
    outs = dict(codes=out_buf(ecodes), pres=out_buf(eres))
    if state is not None:
        outs["state"] = inout((np.asarray(state, np.uint64), ewords))
    return Job("proto", name, b.nseg, b.max_frames, ins, dict(flags=flags, rsv=rsv, limit=limit), outs)


def proto_segments(nseg, mf, seed, flags, limit):
    rng = np.random.default_rng(seed)
    return [PC.random_segment(rng, int(rng.integers(1, mf + 1)), flags, 0, limit, 0.08) for _ in range(nseg)]


def proto_mixed(nseg, mf, seed, limit=7):
    b = PC.Batch(proto_segments(nseg, mf, seed, P.EXPECT_MASKED, limit), mf, gap=seed % 4)
    state = np.zeros(nseg, np.uint64)
    state[::8] = P.ST_OPEN | 2
    return proto_job("mixed %d x %d" % (nseg, mf), b, P.EXPECT_MASKED, 0, limit, state)


def proto_table():
    rows = [r for r in PC.directed_table() if r[2] == P.EXPECT_MASKED and r[3] == 0]
    b = PC.Batch([r[1] for r in rows], max(len(r[1]) for r in rows) + 1, gap=3)
    ecodes = np.full(b.nseg * b.max_frames, FILL, np.uint8)
    eres = np.zeros(b.nseg, P.RES_DTYPE)
    for s, (_n, _f, _fl, _r, codes, first_bad, code, status, close_frame) in enumerate(rows):
        ecodes[s * b.max_frames:s * b.max_frames + len(codes)] = codes
        eres[s] = (first_bad, code, status, close_frame)
    return proto_job("table", b, expect=(ecodes, eres, None))


def proto_jobs():
    period = PC.Batch(proto_segments(50, 40, 33, P.EXPECT_MASKED, 7), 40, gap=1)
    tiled = PC.Tiled(period, 1000)
    return [proto_table(), proto_mixed(43, 6, 30), proto_mixed(57, 9, 31), proto_job("tiled 1000 x 40", tiled, P.EXPECT_MASKED, 0, 7, None),
            proto_mixed(11, 50, 32), proto_mixed(300, 3, 34)]


def proto_hostile():
    """every segment enters with a message open and max_message_size reached, and its frame 0 is a
    continuation with a body: ERR_TOO_BIG at frame 0 everywhere, the smallest first-error keys"""
    nseg, mf, limit = 300, 40, 5
    period = [[PC.error_frame(10, True, limit, limit)] + PC.quiet(mf - 1) for _ in range(3)]
    b = PC.Tiled(PC.Batch(period, mf, gap=1), nseg)
    state = np.full(nseg, P.ST_OPEN | limit, np.uint64)
    exp = P.check(b.dec, b.seg_off, b.desc, b.res, mf, P.EXPECT_MASKED, 0, limit, state)
    return [proto_job("too big at frame 0", b, P.EXPECT_MASKED, 0, limit, state, expect=exp)]


def proto_small():
    return [proto_mixed(7, 60, 40), proto_mixed(45, 4, 41)]


# ------------------------------------------------------------------------------------------ text

POISON = (0xFF, 0xC2, 0xF0)
SENTINEL32 = 0x5A5A5A5A
SEQS = (b"\xc2\xa2", b"\xe2\x82\xac", b"\xf0\x90\x8d\x88")
TEXT_TABLE = [b"", b"a", b"Hello-\xc2\xb5@\xc3\x9f", b"\xce\xba\xe1\xbd\xb9\xcf\x83\xce\xbc\xce\xb5", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
              b"\xc0\xaf", b"\xe0\x80\xaf", b"\xef\xbf\xbd", b"\xf4\x8f\xbf\xbf", b"\x80", b"\xe2\x82", b"\xf0\x90\x8d", b"\xc2", b"\xfe",
              b"text \xe2\x82\xac", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xf0\x8f\xbf\xbf"]


def text_filler(n, seed):
    unit = b"a" + SEQS[0] + b"bc" + SEQS[1] + b"d" + SEQS[2]
    b = (unit * (n // len(unit) + 2))[seed % len(unit):]
    while b and b[0] & 0xC0 == 0x80:
        b = b[1:]
    b = b[:n]
    k = T.tail_start(b)
    return b[:k] + b"x" * (n - k)


def text_job(name, segs, mf, state=None):
    """hand-built d_out / d_msg / d_desc as tests/test_gpu_text.py lays them out: message i of a
    segment takes frame slot i; bodies one after the other, each at a 16-B phase of its own, poison
    bytes between them. segs[s] = [(opcode, body, complete, continued, n_frames)]; state: the words
    in (None: no carry), a pending word standing for one lead byte 0xE2 received so far."""
    nseg = len(segs)
    msg = np.zeros(nseg * mf, W.MSG_DTYPE)
    desc = np.zeros(nseg * mf, W.DESC_DTYPE)
    parts, pos, k = [], 0, 0
    verdict = np.full(nseg * mf, SENTINEL32, np.uint32)
    first_bad = np.zeros(nseg, np.uint32)
    words = None if state is None else np.zeros(nseg, np.uint32)
    for s, ms in enumerate(segs):
        assert len(ms) <= mf
        for i, (opcode, body, complete, continued, n_frames) in enumerate(ms):
            gap = 16 + (k % 16 - (pos + 16)) % 16
            parts.append(np.resize(np.roll(np.array(POISON, np.uint8), k), gap))
            pos += gap
            parts.append(np.frombuffer(bytes(body), np.uint8))
            msg[s * mf + i] = (pos, len(body), i, n_frames, complete, continued)
            desc[s * mf + i]["type"] = 0 if continued else opcode
            desc[s * mf + i]["datalen"] = len(body)
            desc[s * mf + i]["ret"] = 2 + len(body)
            pos += len(body)
            k += 1
        conn = T.TextConn(track=state is not None)
        if state is not None and state[s]:
            assert state[s] == T.state_word(b"\xe2")
            conn.pending, conn.sofar, conn.word = True, b"\xe2", int(state[s])
        v, fb, word = conn.batch(ms)
        verdict[s * mf:s * mf + len(v)] = v
        first_bad[s] = fb
        if words is not None:
            words[s] = word
    parts.append(np.resize(np.array(POISON, np.uint8), 48))
    ins = dict(out=np.concatenate(parts), desc=desc, msg=msg, nmsg=np.array([len(m) for m in segs], np.uint32))
    outs = dict(verdict=out_buf(verdict, 0x5A), first_bad=out_buf(first_bad, 0x5A))
    if state is not None:
        outs["state"] = inout((np.asarray(state, np.uint32), words), 0x5A)
    return Job("text", name, nseg, mf, ins, {}, outs)


def text_mixed(nseg, mf, seed, stated=True):
    rng = np.random.default_rng(seed)
    segs = []
    state = np.zeros(nseg, np.uint32) if stated else None
    for s in range(nseg):
        ms = []
        for i in range(int(rng.integers(0, mf + 1))):
            n = int(rng.choice([0, 1, 15, 16, 17, 63, 200, int(rng.integers(0, 1500))]))
            body = text_filler(n, s + i)
            r = rng.random()
            if r < 0.15 and n:
                body = body[:-1] + b"\xe2"
            elif r < 0.25 and n:
                body = body[:n // 2] + b"\xff" + body[n // 2 + 1:]
            ms.append((int(rng.choice([1, 1, 2])), body, 1, 0, 1 + i % 2))
        if ms and rng.random() < 0.3:
            ms[-1] = ms[-1][:2] + (0,) + ms[-1][3:]
        if ms and stated and rng.random() < 0.3:
            ms[0] = (0, b"\x82\xac" + ms[0][1], ms[0][2], 1, ms[0][4])
            state[s] = T.state_word(b"\xe2")
        segs.append(ms)
    return text_job("mixed %d x %d" % (nseg, mf), segs, mf, state)


def text_table():
    segs = [[(1, v, 1, 0, 1), (1, v, 0, 0, 1), (8, b"\x03\xe8" + v, 1, 0, 1), (2, v, 1, 0, 1)] for v in TEXT_TABLE]
    segs += [[], [(1, b"ok", 1, 0, 1)]]
    return text_job("table", segs, 7, np.zeros(len(segs), np.uint32))


def text_jobs():
    return [text_table(), text_mixed(43, 6, 50), text_mixed(57, 9, 51), text_mixed(1000, 5, 52), text_mixed(11, 50, 53),
            text_mixed(300, 3, 54, stated=False)]


def text_hostile():
    """every slot an open text message that ends in the middle of a sequence, every segment entering
    with a pending message that its first entry continues"""
    nseg, mf = 300, 40
    segs = []
    for s in range(nseg):
        ms = [(1, text_filler(90 + (s + i) % 40, i) + (b"\xe2\x82", b"\xf0\x90", b"\xc2")[i % 3], 0, 0, 1) for i in range(mf)]
        ms[0] = (0, b"\x82\xac" + ms[0][1], 0, 1, 1)
        segs.append(ms)
    return [text_job("open mid-sequence, continued", segs, mf, np.full(nseg, T.state_word(b"\xe2"), np.uint32))]


def text_small():
    return [text_mixed(7, 60, 60), text_mixed(45, 4, 61)]


# ---------------------------------------------------------------------- reassembly and the send list

def rx_batch(nseg, mf, seed, full=False):
    """(wire with PAD bytes behind it, seg_off, seg_len): per segment up to mf (full: exactly mf)
    frames as messages of one to four fragments, text and binary, a few bytes between segments"""
    rng = np.random.default_rng(seed)
    parts, so, sl, pos = [], [], [], 0
    for s in range(nseg):
        left = mf if full else int(rng.integers(0, mf + 1))
        seg = []
        while left:
            n = min(left, int(rng.integers(1, 5)))
            seg.append(RS.message(rng, [int(rng.choice([0, 1, 15, 16, 17, 125, 126, 300])) for _ in range(n)], masked=rng.random() < 0.9,
                                  opcode=1 + s % 2))
            left -= n
        b = b"".join(seg)
        gap = int(rng.integers(0, 20))
        parts.append(b"\xA5" * gap + b)
        so.append(pos + gap)
        sl.append(len(b))
        pos += gap + len(b)
    return np.frombuffer(b"".join(parts) + b"\0" * 64, np.uint8).copy(), so, sl


def reasm_job(name, nseg, mf, seed, full=False):
    wire, so, sl = rx_batch(nseg, mf, seed, full)
    od, orr, oms, oreg, _oop, _oca = oracle_reassemble(wire, so, sl, mf)
    msg = np.zeros(nseg * mf, W.MSG_DTYPE)
    dmask, mmask = np.zeros((nseg * mf, 32), bool), np.zeros((nseg * mf, 32), bool)
    out = np.full(len(wire), FILL, np.uint8)
    for s in range(nseg):
        dmask[s * mf:s * mf + int(orr[s]["n_frames"])] = True
        mmask[s * mf:s * mf + len(oms[s])] = True
        for i, m in enumerate(oms[s]):
            msg[s * mf + i] = m
        ob, body = oreg[s]
        out[ob:ob + len(body)] = body
    ins = dict(buf=wire, seg_off=np.asarray(so, np.uint64), seg_len=np.asarray(sl, np.uint64))
    nmsg = np.array([len(m) for m in oms], np.uint32)
    outs = dict(desc=out_buf(od, mask=dmask), res=out_buf(orr), out=out_buf(out), msg=out_buf(msg, mask=mmask), nmsg=out_buf(nmsg))
    j = Job("reasm", name, nseg, mf, ins, {}, outs, len(wire))
    j.model = (od, orr, oms, out, nmsg, msg)
    return j


def sendlist_expect(od, oms, nseg, mf):
    """the echo's send list from reassembly's descriptors: a complete, not continued text or binary
    message is sent as it is, anything else is a SKIP entry; slots past the count are not written"""
    lst = np.full(nseg * mf * 24, FILL, np.uint8)
    rec = lst.view(S.MSG_DTYPE)
    for s in range(nseg):
        for i, (o, ln, first, _nf, complete, cont) in enumerate(oms[s]):
            t = int(od[s * mf + first]["type"])
            rec[s * mf + i] = (o, ln, t, 0) if complete and not cont and t in (1, 2) else (0, 0, S.SKIP, 0)
    return lst


def sendlist_job(name, nseg, mf, seed):
    r = reasm_job(name, nseg, mf, seed)
    od, _orr, oms, _out, nmsg, msg = r.model
    ins = dict(desc=od, msg=msg, nmsg=nmsg)
    return Job("sendlist", name, nseg, mf, ins, {}, dict(lst=out_buf(sendlist_expect(od, oms, nseg, mf))))


SHAPES = [(24, 12), (43, 6), (57, 9), (1000, 8), (11, 50), (300, 3)]


def reasm_jobs():
    return [reasm_job("rx %d x %d" % s, s[0], s[1], 70 + i) for i, s in enumerate(SHAPES)]


def reasm_hostile():
    return [reasm_job("every segment at max_frames", 1000, 8, 79, full=True)]


def reasm_small():
    return [reasm_job("small 7 x 60", 7, 60, 80), reasm_job("small 45 x 4", 45, 4, 81)]


def sendlist_jobs():
    return [sendlist_job("list %d x %d" % s, s[0], s[1], 90 + i) for i, s in enumerate(SHAPES)]


# ---------------------------------------------------------------------------------------- encode

def encode_job(name, src, frames):
    wire, offs = EC.encode_ref(src, frames)
    ins = dict(src=src, frames=frames)
    return Job("encode", name, len(frames), 1, ins, dict(cap=len(wire)), dict(dst=out_buf(wire, tail=4096), wire_off=out_buf(offs)),
               len(wire))


def encode_mixed(n, seed):
    rng = np.random.default_rng(seed)
    src, fr = EC.counts(n)
    src = rng.integers(0, 256, 8192 + EC.SRC_SLACK, dtype=np.uint8)
    fr["len"] = rng.choice([0, 1, 15, 16, 17, 31, 32, 125, 126, 127, 300, 4000], n)
    return src, fr


def encode_jobs():
    return [encode_job("capacity batch", *EC.capacity_batch()), encode_job("257 frames", *EC.counts(257)),
            encode_job("513 frames", *EC.counts(513)), encode_job("1000 frames of mixed lengths", *encode_mixed(1000, 5)),
            encode_job("piece boundary batch", *EC.capacity_boundary_batch()), encode_job("flags", *EC.flag_batch())]


def encode_hostile():
    return [encode_job("60000 frames", *EC.counts(60000))]


def encode_small():
    return [encode_job("small, long headers", *EC.capacity_batch_long()), encode_job("small, 12 frames", *EC.capacity_batch())]


# ------------------------------------------------------------------- the three workspace-free calls

def handshake_job(name, reqs, exps, flags=0, resp_cap=512):
    buf, so, sl = HC.pack(reqs, align=16)
    nseg = len(reqs)
    hs = np.zeros(nseg, W.HS_DTYPE)
    acc = np.full((nseg, 32), 0x5A, np.uint8)
    resp = np.full(nseg * resp_cap, 0x77, np.uint8)
    for s, x in enumerate(exps):
        rec = HC.expected_record(x, flags, True, resp_cap)
        hs[s] = rec
        if x["ret"] > 0:
            acc[s] = np.frombuffer(x["accept"] + b"\0\0\0\0", np.uint8)
        if rec[6] == W.HS_RESP_WRITTEN:
            r = x["resp_echo"] if flags & HC.ECHO else x["resp"]
            resp[s * resp_cap:s * resp_cap + len(r)] = np.frombuffer(r, np.uint8)
    ins = dict(buf=buf, seg_off=so, seg_len=sl)
    outs = dict(hs=out_buf(hs, 0x77), acc=out_buf(acc, 0x5A), resp=out_buf(resp, 0x77))
    j = Job("handshake", name, nseg, 1, ins, dict(flags=flags, resp_cap=resp_cap), outs, len(buf))
    j.reqs = reqs
    return j


def handshake_table(flags=0):
    with open(os.path.join(HERE, "golden", "handshake_batch.json")) as f:
        rows = json.load(f)
    rows = rows["cases"] if isinstance(rows, dict) else rows
    table = HC.directed_table()
    assert [r["name"] for r in rows] == [n for n, _ in table]
    exps = [{"ret": r["ret"], "key_off": r["key_off"], "key_len": r["key_len"],
             "proto_off": HC.NONE if r["proto_off"] is None else r["proto_off"], "proto_len": r["proto_len"],
             "accept": r["accept"].encode(), "resp": bytes.fromhex(r["resp"]), "resp_echo": bytes.fromhex(r["resp_echo"])}
            for r in rows]
    return handshake_job("table", [d for _n, d in table], exps, flags)


def handshake_jobs():
    host = HC.host_symbols()
    reqs = HC.random_requests(1300)
    out = [handshake_table()]
    for i, n in enumerate((100, 257, 513, 1000, 300)):
        part = reqs[7 * i:7 * i + n]
        out.append(handshake_job("random %d" % n, part, [HC.expected(host, r) for r in part], HC.ECHO if i & 1 else 0, 256 + 64 * i))
    return out


def conn_strings(n):
    return [(b"/" + HC.filler(s % 41, s), (b"", b"chat", b"a, bb ,ccc")[s % 3], (b"", b"h%d.example.com" % s)[s % 2]) for s in range(n)]


def nonces(n, salt=0):
    rng = np.random.default_rng(900 + salt)
    return [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(n)]


def client_request_job(name, n, req_cap, salt=0):
    strings, nn = conn_strings(n), nonces(n, salt)
    strings[n // 2] = (b"/a b", b"", b"")                       # a byte that may not stand in a path
    pool, ent = CC.pool(strings)
    rd = np.zeros(n, W.CLI_REQ_DTYPE)
    req = np.full(n * req_cap, 0x77, np.uint8)
    expect = np.full((n, 32), 0x5A, np.uint8)
    for s, ((path, proto, host), nonce) in enumerate(zip(strings, nn)):
        rec, text, exp = CO.request_record(path, nonce, proto, host, req_cap)
        rd[s] = rec
        if exp is not None:
            expect[s] = np.frombuffer(exp, np.uint8)
        if text is not None:
            req[s * req_cap:s * req_cap + len(text)] = np.frombuffer(text, np.uint8)
    ins = dict(strs=pool, entry=ent, nonce=np.frombuffer(b"".join(nn), np.uint8))
    outs = dict(rd=out_buf(rd, 0x77), req=out_buf(req, 0x77), expect=out_buf(expect, 0x5A))
    j = Job("client_request", name, n, 1, ins, dict(req_cap=req_cap), outs)
    j.strings, j.nonces = strings, nn
    return j


def client_request_jobs():
    return [client_request_job("%d connections" % n, n, cap, i)
            for i, (n, cap) in enumerate(((40, 256), (257, 192), (513, 320), (1000, 256), (64, 100), (300, 512)))]


def client_verify_job(name, cases, max_head=0):
    """cases: (response, offered) pairs, every connection with its own expect value"""
    segs = [d for d, _o in cases]
    buf, so, sl = CC.pack(segs, align=16)
    pool, ent = CC.pool([(b"/", o, b"") for _d, o in cases])
    cv = np.zeros(len(cases), W.CLI_VERIFY_DTYPE)
    for s, (d, o) in enumerate(cases):
        cv[s] = CO.verify(d, CC.EXPECT, o, max_head)
    ins = dict(buf=buf, seg_off=so, seg_len=sl, expect=np.frombuffer(CC.EXPECT * len(cases), np.uint8), strs=pool, entry=ent)
    j = Job("client_verify", name, len(cases), 1, ins, dict(max_head=max_head), dict(cv=out_buf(cv, 0x77)), len(buf))
    j.cases = cases
    return j


def client_verify_jobs():
    table = [(d, o) for _n, d, o, _m in CC.directed_table()]
    mixed = [(d, o) for d, o, m in CC.random_responses(2400, seed=11) if m == 0]
    return [client_verify_job("table", table)] + [client_verify_job("random %d" % n, mixed[3 * i:3 * i + n], 0 if i & 1 else 4000)
                                                  for i, n in enumerate((257, 513, 1000, 100, 300))]


# ------------------------------------------------------------------------------------ the registry

_JOBS = dict(send=send_jobs, reply=reply_jobs, proto=proto_jobs, text=text_jobs, reasm=reasm_jobs, encode=encode_jobs,
             sendlist=sendlist_jobs, handshake=handshake_jobs, client_request=client_request_jobs, client_verify=client_verify_jobs)
_HOSTILE = dict(send=send_hostile, reply=reply_hostile, proto=proto_hostile, text=text_hostile, reasm=reasm_hostile,
                encode=encode_hostile)
_SMALL = dict(send=send_small, reply=reply_small, proto=proto_small, text=text_small, reasm=reasm_small, encode=encode_small)


@functools.lru_cache(maxsize=None)
def _all(kind):
    return tuple(_JOBS[kind]())


def jobs(kind, n=6):
    """n jobs of `kind`, largest first when sorted by the caller; built once and never modified"""
    a = _all(kind)
    assert n <= len(a)
    return list(a[:n])


@functools.lru_cache(maxsize=None)
def hostile(kind):
    return tuple(_HOSTILE[kind]())


@functools.lru_cache(maxsize=None)
def small(kind):
    return tuple(_SMALL[kind]())
