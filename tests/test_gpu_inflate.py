"""websocketframeBatchInflateDevice and websocketframeBatchInflateListFromMessagesDevice on the device,
bit for bit against the sequential model (inflate_oracle.py: CPython's zlib per message, first
failure, NOT_RUN, the packing): d_msg_res, d_res, every region's [0, out_len), and a sentinel fill
outside the regions and behind every array untouched."""
import zlib

import numpy as np
import pytest

import inflate_cases as IC
import inflate_oracle as O
from oracle_lib import oracle_reassemble
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GAP = 48                          # sentinel bytes between and behind the regions


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def place(bodies, aligns=None):
    """bodies into one source buffer, body k starting at an address that is aligns[k] mod 16 (the
    buffer itself is 256-B aligned on the device), a sentinel between them: (src, [(off, len)])"""
    parts, at, spans = [], 0, []
    for k, b in enumerate(bodies):
        a = 0 if aligns is None else aligns[k]
        pad = (a - at) % 16 + 16
        parts.append(bytes([O.FILL]) * pad)
        at += pad
        spans.append((at, len(b)))
        parts.append(b)
        at += len(b)
    return np.frombuffer(b"".join(parts) + bytes([O.FILL]) * 16, np.uint8).copy(), spans


class Call:
    """the device buffers of one batch. conns: per connection [(src_off, len, kind)]; caps: every
    connection's room (default: what its messages need); odd: region offsets that are no multiple of 16;
    offs: every connection's region offset, ascending and at least GAP apart (default: packed)"""

    def __init__(self, dev, src, conns, limit=0, caps=None, max_msgs=None, nmsg=None, odd=False, src_t=None, offs=None):
        self.dev, self.nseg, self.limit = dev, len(conns), limit
        self.mm = max_msgs or max([1] + [len(c) for c in conns])
        msg = np.zeros(self.nseg * self.mm, O.MSG_DTYPE)
        for s, c in enumerate(conns):
            for i, e in enumerate(c[:self.mm]):
                msg[s * self.mm + i] = e + (0,)
        self.nmsg = np.array([len(c) for c in conns] if nmsg is None else nmsg, np.uint32)
        if caps is None:
            caps = []
            for c in conns:
                caps.append(sum(len(O.inflate_one(bytes(src[o:o + n]), limit)[1]) for o, n, k in c[:self.mm]
                                if k == O.RAW and o + n <= len(src)))
        self.caps = np.array(caps, np.uint64)
        if offs is None:
            offs, at = [], GAP + (5 if odd else 0)
            for s in range(self.nseg):
                offs.append(at)
                at += int(self.caps[s]) + GAP + ((3 + 2 * s) % 16 if odd else 0)
        else:
            at = GAP
            for s in range(self.nseg):
                assert int(offs[s]) >= at, "region %d overlaps the one before it or its sentinels" % s
                at = int(offs[s]) + int(self.caps[s]) + GAP
        self.offs = np.array(offs, np.uint64)
        self.exp = O.batch(src, msg, self.nmsg, self.mm, limit, self.offs, self.caps, fill=O.FILL)
        self.src = T(src, dev) if src_t is None else src_t
        self.msg, self.nmsg_t = T(msg, dev), T(self.nmsg, dev).view(torch.int32)
        self.dst = torch.full((at + GAP,), O.FILL, dtype=torch.uint8, device=dev)
        self.off_t, self.cap_t = T(self.offs, dev).view(torch.int64), T(self.caps, dev).view(torch.int64)
        self.mres = torch.full((24 * self.nseg * self.mm + 24,), O.FILL, dtype=torch.uint8, device=dev)
        self.res = torch.full((24 * self.nseg + 24,), O.FILL, dtype=torch.uint8, device=dev)

    def refill(self):
        for t in (self.dst, self.mres, self.res):
            t.fill_(O.FILL)

    def run(self, stream=None):
        W.batch_inflate_device(self.src, self.msg, self.nmsg_t, self.mm, self.dst, self.off_t, self.cap_t,
                               self.mres[:24 * self.nseg * self.mm], self.res[:24 * self.nseg], max_message_size=self.limit,
                               stream=stream)

    def check(self, tag=""):
        torch.cuda.synchronize()
        emr, eres, outs = self.exp
        mres, res, dst = self.mres.cpu().numpy(), self.res.cpu().numpy(), self.dst.cpu().numpy()
        print(tag, "connections", self.nseg, "inflated", int(eres["out_len"].sum()), "statuses", np.bincount(eres["status"], minlength=5))
        got = res[:24 * self.nseg].view(O.RES_DTYPE)
        bad = np.flatnonzero(got != eres)
        assert len(bad) == 0, "%s: connection %d: %s, expected %s" % (tag, bad[0], got[bad[0]], eres[bad[0]])
        assert (res[24 * self.nseg:] == O.FILL).all(), tag + ": bytes behind d_res written"
        gm = mres[:24 * self.nseg * self.mm].view(O.MSGRES_DTYPE)
        bad = np.flatnonzero(gm != emr)
        assert len(bad) == 0, "%s: slot %d: %s, expected %s" % (tag, bad[0], gm[bad[0]], emr[bad[0]])
        assert (mres[24 * self.nseg * self.mm:] == O.FILL).all(), tag + ": bytes behind d_msg_res written"
        at = 0
        for s in range(self.nseg):
            lo, cap = int(self.offs[s]), int(self.caps[s])
            assert (dst[at:lo] == O.FILL).all(), "%s: bytes before region %d written" % (tag, s)
            want = np.frombuffer(outs[s], np.uint8)
            wrong = np.flatnonzero(dst[lo:lo + len(want)] != want)
            assert len(wrong) == 0, "%s: connection %d: first wrong byte at %d of %d" % (tag, s, wrong[0], len(want))
            at = lo + cap
        assert (dst[at:] == O.FILL).all(), tag + ": bytes behind the last region written"


def one_per_connection(spans):
    return [[(o, n, O.RAW)] for o, n in spans]


@pytest.fixture(scope="module")
def table():
    return IC.directed_table()


def test_directed_table_as_one_batch(dev, table):
    src, spans = place([b for _, b in table])
    c = Call(dev, src, one_per_connection(spans))
    c.run()
    c.check("directed")
    assert {O.OK, O.ERR_DATA} == set(int(v) for v in c.exp[1]["status"])


@pytest.mark.parametrize("half", [0, 1])
def test_every_source_alignment_and_odd_regions(dev, table, half):
    bodies = [b for _, b in table if len(b) < 5000]
    al = [(k + 8 * half) % 16 for k in range(len(bodies))]
    reps = []
    for a in range(8 * half, 8 * half + 8):               # every body at 8 alignments per half: all 16 over both
        reps += [(b, (x + a) % 16) for b, x in zip(bodies, al)]
    src, spans = place([b for b, _ in reps], [a for _, a in reps])
    assert {(o % 16) for o, _ in spans} == set(range(16))
    c = Call(dev, src, one_per_connection(spans), odd=True)
    assert any(int(o) % 16 for o in c.offs)
    c.run()
    c.check("alignments")


def test_truncations_and_bit_flips(dev):
    bodies = IC.truncations()[::3] + IC.bit_flips()[::2]
    src, spans = place(bodies)
    c = Call(dev, src, one_per_connection(spans))
    c.run()
    c.check("mutations")


def mixed_batch(nconn=300, seed=5):
    """connections of 0-5 entries: RAW, SKIP and failing entries at every position, counts past
    max_msgs, rooms with no spare byte and one byte short, the limit one below, at and above a size"""
    rng = np.random.default_rng(seed)
    good = [IC.deflate(IC.text(rng, int(n)), int(lv)) for n, lv in zip(rng.integers(0, 1500, 40), rng.choice([0, 1, 6, 9], 40))]
    limit = max(len(O.inflate_one(b)[1]) for b in good) + 2
    good.append(IC.deflate(b"w" * (limit - 1), 6))        # the limit one above the message's size,
    good.append(IC.deflate(b"x" * limit, 6))              # at it,
    good.append(IC.deflate(b"y" * (limit + 1), 6))        # and one below: too big
    bad = [b for _, b, meant in IC.hand_built() if meant is None]
    src, spans = place(good + bad)
    gs, bs = spans[:len(good)], spans[len(good):]
    conns, nmsg, caps = [], [], []
    for s in range(nconn):
        n = int(rng.integers(0, 6))
        lst = []
        for i in range(n):
            u = rng.random()
            if u < 0.2:
                lst.append((0, 0, O.SKIP) if u < 0.1 else (len(src) + 5, 1 << 40, O.SKIP))
            else:
                lst.append(gs[int(rng.integers(0, len(gs)))] + (O.RAW,))
        if n and s % 3 == 0:                              # a failing entry first, in the middle or last
            at = [0, n // 2, n - 1][(s // 3) % 3]
            kind = (s // 9) % 3
            lst[at] = (bs[s % len(bs)] + (O.RAW,) if kind == 0 else
                       ((len(src) - 3, 4, O.RAW) if kind == 1 else (0, 0, 7)))
        conns.append(lst)
        nmsg.append(n + (3 if s % 7 == 0 else 0))         # past the list and, for n = 5, past max_msgs
        need = sum(len(O.inflate_one(bytes(src[o:o + ln]), limit)[1]) for o, ln, k in lst[:4] if k == O.RAW and o + ln <= len(src))
        caps.append(max(0, need - 1) if s % 5 == 1 else need + (0 if s % 2 else 9))
    return src, conns, nmsg, caps, limit


def test_mixed_connections(dev):
    src, conns, nmsg, caps, limit = mixed_batch()
    # nmsg counts entries the list may not have: pad every list to 8 with SKIPs, clip at max_msgs 4
    conns = [c + [(0, 0, O.SKIP)] * (8 - len(c)) for c in conns]
    c = Call(dev, src, conns, limit=limit, caps=caps, max_msgs=4, nmsg=nmsg)
    st = set(int(v) for v in c.exp[1]["status"])
    assert st == {O.OK, O.ERR_DATA, O.ERR_TOO_BIG, O.ERR_OUT_SPACE, O.ERR_RANGE}, st
    assert (c.exp[0]["status"] == O.NOT_RUN).any() and (np.array(nmsg) > 4).any()
    c.run()
    c.check("mixed")


@pytest.mark.parametrize("limit", [1998, 1999, 2000, 2001])
def test_limit_beside_an_error(dev, limit):
    """2000 good bytes, then a block of type 3, beside good messages of 1999-2001 bytes: with room for
    limit + 1 bytes zlib reaches the bad block from limit 1999 on; rooms of the exact size and one short"""
    rng = np.random.default_rng(12)
    data = IC.text(rng, 3000)
    bodies = [IC.deflate(data[:2000], 6) + O.TAIL + bytes([7])] + [IC.deflate(data[:n], lv) for n in (1999, 2000, 2001) for lv in (0, 6)]
    src, spans = place(bodies * 2)
    caps = [2000] * 7 + [1999] * 7
    c = Call(dev, src, one_per_connection(spans), limit=limit, caps=caps)
    assert int(c.exp[1]["status"][0]) == (O.ERR_TOO_BIG if limit < 1999 else O.ERR_DATA)
    c.run()
    c.check("limit %d" % limit)


def test_one_long_message_beside_63_small(dev):
    rng = np.random.default_rng(2)
    big = IC.text(rng, 1 << 20) + rng.integers(0, 256, 1 << 19, dtype=np.uint8).tobytes() + IC.text(rng, 1 << 19)
    bodies = [IC.deflate(IC.text(rng, 200 + k), 6) for k in range(63)]
    bodies.insert(17, IC.deflate(big, 6))
    src, spans = place(bodies)
    c = Call(dev, src, one_per_connection(spans))
    c.run()
    c.check("long")
    assert int(c.exp[1]["out_len"][17]) == 1 << 21


def test_every_connection_fails_at_its_first_entry(dev):
    bad = [b for _, b, meant in IC.hand_built() if meant is None]
    src, spans = place(bad + [IC.deflate(b"fine", 6)])
    good = spans[-1] + (O.RAW,)
    conns = [[spans[k] + (O.RAW,), good, good] for k in range(len(bad))]
    c = Call(dev, src, conns)
    c.run()
    c.check("all fail")
    assert (c.exp[1]["first_bad"] == 0).all() and (c.exp[1]["close_status"] == 1007).all()


def test_no_connection_and_one(dev):
    src, spans = place([IC.deflate(b"Hello, hello, hello", 6)])
    c = Call(dev, src, one_per_connection(spans))
    c.run()
    c.check("one")
    c.refill()
    W.batch_inflate_device(c.src, c.msg, c.nmsg_t[:0], 1, c.dst, c.off_t[:0], c.cap_t[:0], c.mres[:24], c.res[:24])
    torch.cuda.synchronize()
    for t in (c.dst, c.mres, c.res):
        assert bool((t == O.FILL).all())


def test_non_default_stream_and_two_streams(dev, table):
    src, spans = place([b for _, b in table if len(b) < 3000])
    a = Call(dev, src, one_per_connection(spans))
    b = Call(dev, src, one_per_connection(spans[::-1]), odd=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a.run(s1)
    with torch.cuda.stream(s2):
        b.run(s2)
    a.check("stream 1")
    b.check("stream 2")


def test_captured_call_replayed_twice(dev, table):
    src, spans = place([b for _, b in table if len(b) < 3000])
    c = Call(dev, src, one_per_connection(spans))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c.run(st)                                         # the warm call
        c.check("warm")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            c.run(st)
    for k in range(2):
        c.refill()
        torch.cuda.synchronize()
        g.replay()
        c.check("replay %d" % k)


def frame(opcode, fin, rsv1, body, key):
    b0 = (0x80 if fin else 0) | (0x40 if rsv1 else 0) | opcode
    n = len(body)
    h = bytes([b0, 0x80 | n]) if n < 126 else (bytes([b0, 0x80 | 126]) + n.to_bytes(2, "big") if n < 65536 else
                                               bytes([b0, 0x80 | 127]) + n.to_bytes(8, "big"))
    k = key.to_bytes(4, "little")
    return h + k + bytes(v ^ k[i & 3] for i, v in enumerate(body))


def test_map_and_chain_end_to_end(dev):
    """compressed and plain messages as masked frames with and without RSV1, over 1-3 frames, beside
    control frames, a message left open and messages continued from an earlier batch (d_open): the
    map slot by slot, and reassemble -> map -> inflate gives the original messages"""
    rng = np.random.default_rng(8)
    mf, wires, plans = 16, [], []
    for s in range(6):
        wire, plan = b"", []
        for i in range(4):
            data = IC.text(rng, int(rng.integers(1, 900)))
            comp = (s + i) % 3 != 0
            body = IC.deflate(data, 6) if comp else data
            nf = 1 + (s + i) % 3
            cuts = [len(body) * j // nf for j in range(nf + 1)]
            for j in range(nf):
                wire += frame((1 + i % 2) if j == 0 else 0, j == nf - 1, comp and j == 0, body[cuts[j]:cuts[j + 1]], 0x01020304 * (i + 1))
            if i == 1:
                wire += frame(9, True, False, b"ping", 77)          # a control frame between two messages
            plan.append((comp, data))
        if s % 2:
            wire += frame(2, False, True, b"\x00open", 5)         # a compressed message still open at the batch end
        wires.append(wire)
        plans.append(plan)
    # connections with a message open from an earlier batch: its first frame in this batch is a
    # continuation that closes it (6), one that leaves it open (7), and — a peer that breaks the
    # protocol — a text frame with RSV1 that closes it (8): continued, so never inflated
    late = IC.text(rng, 300)
    wires.append(frame(0, True, False, b"the rest of an earlier message", 9) + frame(1, True, True, IC.deflate(late, 6), 10))
    wires.append(frame(0, False, False, b"more of an earlier message", 11))
    wires.append(frame(1, True, True, IC.deflate(b"joins the open message", 6), 12) + frame(2, True, True, IC.deflate(late, 9), 13))
    nc, open_in = len(wires), [0] * 6 + [1, 1, 1]
    so, at = [], 0
    for w in wires:
        so.append(at)
        at += len(w) + 11
    wire = np.full(at, 0, np.uint8)
    for o, w in zip(so, wires):
        wire[o:o + len(w)] = np.frombuffer(w, np.uint8)
    sl = [len(w) for w in wires]
    oo = [o + 64 for o in so]
    od, orr, oms, oreg, _, _ = oracle_reassemble(wire.copy(), so, sl, mf, open_in=open_in, out_off=oo)
    n = len(wire)
    d = torch.zeros(n + W.BATCH_PAD, dtype=torch.uint8, device=dev)
    d[:n] = T(wire, dev)
    out = torch.full((n + 512,), 0x55, dtype=torch.uint8, device=dev)
    desc = torch.zeros(nc * 32 * mf, dtype=torch.uint8, device=dev)
    res = torch.zeros(nc * 16, dtype=torch.uint8, device=dev)
    msg = torch.zeros(nc * 32 * mf, dtype=torch.uint8, device=dev)
    nmsg = torch.zeros(nc, dtype=torch.int32, device=dev)
    t64 = lambda a: T(np.array(a, np.uint64), dev).view(torch.int64)  # noqa: E731
    W.batch_reassemble_device(d, t64(so), t64(sl), mf, desc, res, out, msg, nmsg, out_off=t64(oo),
                              open_state=T(np.array(open_in, np.uint8), dev))
    lst = T(np.full(nc * mf * 24 + 24, O.FILL, np.uint8), dev)
    W.batch_inflate_list_from_messages_device(d, desc, msg, nmsg, mf, lst[:nc * 24 * mf])
    torch.cuda.synchronize()
    got = lst.cpu().numpy()
    assert (got[nc * 24 * mf:] == O.FILL).all()
    body = out.cpu().numpy()
    conns, kinds = [], set()
    for s in range(nc):
        want = []
        for (o, ln, first, _nf, complete, cont) in oms[s]:
            t = int(od[s * mf + first]["type"])
            rsv1 = bool(wire[int(od[s * mf + first]["frame_off"])] & 0x40)
            raw = complete and not cont and t in (1, 2) and rsv1
            kinds.add((bool(complete), bool(cont), t in (1, 2), rsv1))
            want.append((o, ln, O.RAW) if raw else (0, 0, O.SKIP))
        want += [(0, 0, O.SKIP)] * (mf - len(want))
        rec = got[s * 24 * mf:(s + 1) * 24 * mf].view(O.MSG_DTYPE)
        assert [(int(r["src_off"]), int(r["len"]), int(r["kind"])) for r in rec] == want and not rec["reserved"].any(), s
        conns.append(want)
    # (complete, continued, data opcode, RSV1): compressed, plain, control, open; continued and closed,
    # continued and open, continued with a data opcode and RSV1 on its first frame here
    assert {(True, False, True, True), (True, False, True, False), (True, False, False, False), (False, False, True, True),
            (True, True, False, False), (False, True, False, False), (True, True, True, True)} <= kinds
    for s in (6, 7, 8):
        assert oms[s][0][5] == 1 and conns[s][0] == (0, 0, O.SKIP), "a continued message is never inflated"
    # inflate with d_out as d_src, d_nmsg and max_frames reused
    c = Call(dev, body, conns, max_msgs=mf, nmsg=nmsg.cpu().numpy().view(np.uint32), src_t=out)
    c.msg = lst
    c.run()
    c.check("chain")
    for s in range(6):
        texts = [data for comp, data in plans[s] if comp]
        assert c.exp[2][s] == b"".join(texts) and int(c.exp[1][s]["n_msgs"]) == len(texts)
        plain = [data for comp, data in plans[s] if not comp]
        for (o, ln, first, _nf, complete, cont), (comp, data) in zip([m for m in oms[s] if int(od[s * mf + m[2]]["type"]) in (1, 2)], plans[s]):
            if not comp:
                assert bytes(body[o:o + ln]) == data
        assert plain or texts
    assert c.exp[2][6] == late and c.exp[2][7] == b"" and c.exp[2][8] == late


def test_argument_errors_launch_nothing(dev):
    src, spans = place([IC.deflate(b"Hello, hello, hello", 6)])
    c = Call(dev, src, one_per_connection(spans))
    lib = _lib.load_deflate_lib()
    p = dict(src=c.src.data_ptr(), n=c.src.numel(), msg=c.msg.data_ptr(), nmsg=c.nmsg_t.data_ptr(), nseg=1, mm=1, limit=0, flags=0,
             dst=c.dst.data_ptr(), off=c.off_t.data_ptr(), cap=c.cap_t.data_ptr(), mres=c.mres.data_ptr(), res=c.res.data_ptr())

    def call(**kw):
        a = dict(p, **kw)
        return lib.websocketframeBatchInflateDevice(a["src"], a["n"], a["msg"], a["nmsg"], a["nseg"], a["mm"], a["limit"], a["flags"],
                                                    a["dst"], a["off"], a["cap"], a["mres"], a["res"], None)
    for kw, word in ([(dict([(k, None)]), b"NULL") for k in ("src", "msg", "nmsg", "dst", "off", "cap", "mres", "res")] +
                     [(dict(mm=0), b"max_msgs"), (dict(flags=1), b"flag"), (dict(msg=p["msg"] + 4), b"aligned"),
                      (dict(res=p["res"] + 4), b"aligned"), (dict(nmsg=p["nmsg"] + 2), b"aligned"),
                      (dict(nseg=1 << 16, mm=(1 << 14) + 1), b"2^30")]):
        assert call(**kw) < 0 and word in lib.websocketframeGpuLastError(), kw
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    assert lib.websocketframeBatchInflateListFromMessagesDevice(None, d.data_ptr(), d.data_ptr(), d.data_ptr(), 1, 1, d.data_ptr(), None) < 0
    assert lib.websocketframeBatchInflateListFromMessagesDevice(d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), 1, 0, d.data_ptr(), None) < 0
    torch.cuda.synchronize()
    for t in (c.dst, c.mres, c.res):
        assert bool((t == O.FILL).all())
    c.run()
    c.check("after the refusals")
    assert zlib.decompressobj(-15).decompress(bytes(src[spans[0][0]:spans[0][0] + spans[0][1]]) + O.TAIL) == c.exp[2][0]
