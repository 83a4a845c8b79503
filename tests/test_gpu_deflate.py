"""websocketframeBatchDeflateDevice, websocketframeBatchSendListFromDeflatedDevice and
websocketframeBatchSendExtDevice on the device. The deflate rule is deterministic, so the device is
held byte for byte against the host twin (websocketframeDeflateHost, itself judged by zlib in
test_deflate_host.py): d_msg_res, every room, sentinels around the rooms and behind every array;
the map against deflate_oracle.send_entry; the ext send against send_oracle's bytes with 0x40 on
first frames; and the whole chain back through reassembly and the inflate to the originals."""
import numpy as np
import pytest

import deflate_cases as DC
import deflate_oracle as O
import high_arena as H
import inflate_cases as IC
import send_cases as SC
import send_oracle as S
from util_amd import _lib
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GAP = 40                          # sentinel bytes between and behind the rooms
NONE64 = 0xEEEEEEEEEEEEEEEE


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


def place(bodies, aligns=None):
    """bodies into one source buffer, body k at an address that is aligns[k] mod 16: (src, [(off, len)])"""
    parts, at, spans = [], 0, []
    for k, b in enumerate(bodies):
        a = k % 16 if aligns is None else aligns[k]
        pad = (a - at) % 16 + 16
        parts.append(bytes([0x5A]) * pad)
        at += pad
        spans.append((at, len(b)))
        parts.append(b)
        at += len(b)
    return np.frombuffer(b"".join(parts) + bytes([0x5A]) * 16, np.uint8).copy(), spans


def host_twin(src, msg, nmsg, mm, min_len, dst_len, offs, caps, src_len=None):
    """websocketframeDeflateHost connection by connection into one destination image: (dst, mres bytes)"""
    lib = _lib.load_pmd_lib()
    dst = np.full(dst_len, O.FILL, np.uint8)
    mres = np.full(24 * len(nmsg) * mm + 24, O.FILL, np.uint8)
    for s in range(len(nmsg)):
        n = min(int(nmsg[s]), mm)
        if n == 0:
            continue
        m, o, c = msg[s * mm:s * mm + n].copy(), offs[s * mm:s * mm + n].copy(), caps[s * mm:s * mm + n].copy()
        r = np.zeros(n, O.MSGRES_DTYPE)
        rc = lib.websocketframeDeflateHost(src.ctypes.data, len(src) if src_len is None else src_len, m.ctypes.data, n, min_len, 0,
                                           dst.ctypes.data, o.ctypes.data, c.ctypes.data, r.ctypes.data)
        assert rc >= 0
        mres[24 * s * mm:24 * (s * mm + n)] = r.view(np.uint8)
    return dst, mres


class Call:
    """the device buffers of one deflate batch. conns: per connection [(src_off, len, type)]; caps: per
    slot (default max(len, 1) for entries in range, 8 otherwise); rooms at odd offsets"""

    def __init__(self, dev, src, conns, min_len=0, caps=None, max_msgs=None, nmsg=None):
        self.dev, self.nseg, self.min_len, self.src_np = dev, len(conns), min_len, src
        self.mm = max_msgs or max([1] + [len(c) for c in conns])
        self.msg_np = np.zeros(self.nseg * self.mm, O.MSG_DTYPE)
        self.msg_np["src_off"], self.msg_np["len"], self.msg_np["type"] = 1 << 50, 1 << 50, 3     # poison past the counts
        for s, c in enumerate(conns):
            for i, e in enumerate(c[:self.mm]):
                self.msg_np[s * self.mm + i] = e + (0,)
        self.nmsg_np = np.array([len(c) for c in conns] if nmsg is None else nmsg, np.uint32)
        q = self.nseg * self.mm
        if caps is None:
            caps = [max(int(m["len"]), 1) if int(m["len"]) <= len(src) else 8 for m in self.msg_np]
        self.caps = np.array(caps, np.uint64)
        offs, at = [], GAP + 3
        for k in range(q):
            offs.append(at)
            at += int(self.caps[k]) + GAP + (5 * k) % 16
        self.offs, self.dst_len = np.array(offs, np.uint64), at + GAP
        self.exp = host_twin(src, self.msg_np, self.nmsg_np, self.mm, min_len, self.dst_len, self.offs, self.caps)
        self.src = T(src, dev)
        self.msg, self.nmsg = T(self.msg_np, dev), T(self.nmsg_np, dev).view(torch.int32)
        self.dst = torch.full((self.dst_len,), O.FILL, dtype=torch.uint8, device=dev)
        self.off_t, self.cap_t = T(self.offs, dev).view(torch.int64), T(self.caps, dev).view(torch.int64)
        self.mres = torch.full((24 * q + 24,), O.FILL, dtype=torch.uint8, device=dev)

    def run(self, stream=None):
        W.batch_deflate_device(self.src, self.msg, self.nmsg, self.mm, self.dst, self.off_t, self.cap_t,
                               self.mres[:24 * self.nseg * self.mm], min_len=self.min_len, stream=stream)

    def records(self):
        return self.exp[1][:24 * self.nseg * self.mm].view(O.MSGRES_DTYPE)

    def check(self, tag=""):
        torch.cuda.synchronize()
        edst, emres = self.exp
        mres, dst = self.mres.cpu().numpy(), self.dst.cpu().numpy()
        bad = np.flatnonzero(mres != emres)
        assert len(bad) == 0, "%s: d_msg_res differs at slot %d: %s, host %s" % (
            tag, bad[0] // 24, mres[bad[0] // 24 * 24:][:24].view(O.MSGRES_DTYPE), emres[bad[0] // 24 * 24:][:24].view(O.MSGRES_DTYPE))
        bad = np.flatnonzero(dst != edst)
        assert len(bad) == 0, "%s: d_dst differs from the host twin's at %d (%d bytes)" % (tag, bad[0], len(bad))
        assert bool((self.src.cpu() == torch.from_numpy(self.src_np)).all()), tag + ": d_src written"
        st = self.records()["status"]
        live = np.concatenate([np.arange(s * self.mm, s * self.mm + min(int(n), self.mm)) for s, n in enumerate(self.nmsg_np)] or
                              [np.zeros(0, int)]).astype(int)
        print(tag, "slots", len(live), "statuses", np.bincount(st[live], minlength=5))
        return st[live]


def ragged(spans, rng, types=(1, 2)):
    """the spans dealt to connections of 0 to 4 entries"""
    conns, k = [], 0
    while k < len(spans):
        n = int(rng.integers(0, 5))
        conns.append([spans[k + i] + (types[(k + i) % len(types)],) for i in range(min(n, len(spans) - k))])
        k += n
    return conns


@pytest.fixture(scope="module")
def table():
    return DC.directed_table()


def test_parity_directed_table_and_sweep(dev, table):
    """every directed body and 200 sweep bodies, at every source alignment, as connections with
    ragged counts (some past max_msgs, some short of their lists)"""
    bodies = [b for _, b in table] + DC.sweep(200, seed=31, max_len=20000)
    src, spans = place(bodies)
    assert {o % 16 for o, _ in spans} == set(range(16))
    rng = np.random.default_rng(1)
    conns = ragged(spans, rng)
    nmsg = [len(c) + (2 if s % 5 == 0 else 0) - (1 if s % 7 == 3 and len(c) > 1 else 0) for s, c in enumerate(conns)]
    c = Call(dev, src, conns, max_msgs=4, nmsg=nmsg)
    assert (np.array(nmsg) > 4).any()
    c.run()
    st = c.check("parity")
    assert {O.DEFLATED, O.PLAIN} <= set(int(v) for v in st)
    # what the host twin wrote is what zlib reads: one DEFLATED room, end to end
    r = c.records()
    q = int(np.flatnonzero(r["status"] == O.DEFLATED)[-1])
    m = c.msg_np[q]
    room = c.dst.cpu().numpy()[int(r[q]["out_off"]):][:int(r[q]["out_len"])]
    assert O.inflate(room) == bytes(src[int(m["src_off"]):int(m["src_off"]) + int(m["len"])])


def test_verdict_edges(dev):
    """cap at out_len - 1 and out_len for a DEFLATED and a PLAIN message, min_len at len - 1, len and
    len + 1, ERR_RANGE one byte past the source, SKIP between live entries"""
    good, rand = IC.text(np.random.default_rng(2), 700), DC.rnd(3, 700)
    src = np.frombuffer(good + rand, np.uint8).copy()
    n = len(src)
    _, mr, _ = W.deflate_host(src, np.array([(0, 700, 1, 0)], W.DEFLATE_MSG_DTYPE), [0], [700], 700)
    z = int(mr[0]["out_len"])
    assert int(mr[0]["status"]) == O.DEFLATED and z < 700
    skip = (n + 9, 1 << 44, O.SKIP)
    conns = [[(0, 700, 1), (0, 700, 1), skip, (0, 700, 2), (700, 700, 1), (700, 700, 2)],
             [(0, 699, 1), skip, (0, 700, 1), (0, 701, 1), (0, 0, 2)],
             [(n - 4, 5, 1), (n - 5, 5, 1), (1 << 63, 1 << 63, 2), skip, (n, 0, 1), (n + 1, 0, 1)]]
    caps = [z, z - 1, 4, 5000, 700, 699,
            699, 4, 700, 701, 0, 8,
            8, 8, 8, 8, 0, 8]
    c = Call(dev, src, conns, min_len=700, caps=caps)
    c.run()
    c.check("edges")
    want = [O.DEFLATED, O.ERR_OUT_SPACE, O.SKIPPED, O.DEFLATED, O.PLAIN, O.ERR_OUT_SPACE,
            O.PLAIN, O.SKIPPED, O.DEFLATED, O.DEFLATED, O.PLAIN, None,
            O.ERR_RANGE, O.PLAIN, O.ERR_RANGE, O.SKIPPED, O.PLAIN, O.ERR_RANGE]
    got = [int(v) for v in c.records()["status"]]
    assert [g for g, w in zip(got, want) if w is not None] == [w for w in want if w is not None]
    c2 = Call(dev, src, [[(0, 700, 1)], [(0, 700, 1)], [(0, 700, 1)]][:3], min_len=701)
    c2.run()
    assert [int(v) for v in c2.check("min_len above")] == [O.PLAIN] * 3
    c3 = Call(dev, src, [[(0, 700, 1)]], min_len=699)
    c3.run()
    assert [int(v) for v in c3.check("min_len below")] == [O.DEFLATED]


def test_map_slot_by_slot(dev):
    mm, nseg = 6, 4
    res = np.zeros(nseg * mm, O.MSGRES_DTYPE)
    msg = np.zeros(nseg * mm, O.MSG_DTYPE)
    for q in range(nseg * mm):
        res[q] = (1000 + q, 50 + q, q % 5, 0)
        msg[q] = (7, 9, [1, 2, O.SKIP, 0x1F2][q % 4], 0)
    nmsg = np.array([6, 3, 0, 9], np.uint32)
    out = T(np.full(24 * nseg * mm + 24, O.FILL, np.uint8), dev)
    W.batch_send_list_from_deflated_device(T(msg, dev), T(nmsg, dev).view(torch.int32), mm, T(res, dev), out[:24 * nseg * mm])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[24 * nseg * mm:] == O.FILL).all()
    seen = set()
    for s in range(nseg):
        for i in range(mm):
            q = s * mm + i
            rec = got[24 * q:24 * q + 24]
            if i >= min(int(nmsg[s]), mm):
                assert (rec == O.FILL).all(), "slot past the count written"
                continue
            r = rec.view(O.MSG_DTYPE)[0]
            want = O.send_entry(int(msg[q]["type"]), int(res[q]["status"]), 1000 + q, 50 + q)
            assert (int(r["src_off"]), int(r["len"]), int(r["type"])) == want and int(r["reserved"]) == 0, q
            seen.add((int(res[q]["status"]), want[2] == O.SKIP))
    assert {(st, st >= 2) for st in range(5)} <= seen


class SendCall:
    """one ext-send batch against O.send_ext (or the plain send, ext=False)"""

    def __init__(self, dev, src, conns, frags, keys, mm, flags=1, src_t=None):
        self.nseg, self.mm, self.flags = len(conns), mm, flags
        msg, nmsg, _ = S.pack(conns, mm)
        self.exp = O.send_ext(src, conns, frags, keys, mm, flags)
        self.total = int(self.exp[1][-1])
        self.src = T(src, dev) if src_t is None else src_t
        self.msg, self.nmsg = T(msg, dev), T(nmsg, dev).view(torch.int32)
        self.frags = None if frags is None else T(np.asarray(frags, np.uint32), dev).view(torch.int32)
        self.keys = None if keys is None else T(keys, dev).view(torch.int32)
        self.tx = torch.full((self.total + 64,), S.FILL, dtype=torch.uint8, device=dev)
        self.tx_off = T(np.full(self.nseg + 2, NONE64, np.uint64), dev).view(torch.int64)
        self.res = T(np.full(self.nseg * 32 + 32, S.FILL, np.uint8), dev)

    def run(self, ext=True, stream=None):
        fn = W.batch_send_ext_device if ext else W.batch_send_device
        fn(self.src, self.msg, self.nmsg, self.mm, self.tx[:self.total], self.tx_off[:self.nseg + 1], self.res[:32 * self.nseg],
           frag_size=self.frags, mask_key=self.keys, tx_capacity=self.total, flags=self.flags if ext else 0, stream=stream)

    def check(self, tag=""):
        torch.cuda.synchronize()
        etx, eoff, _, eres = self.exp
        assert np.array_equal(self.tx_off.cpu().numpy().view(np.uint64)[:self.nseg + 1], eoff), tag
        assert np.array_equal(self.res.cpu().numpy()[:32 * self.nseg].view(S.RES_DTYPE), eres), tag
        buf = self.tx.cpu().numpy()
        bad = np.flatnonzero(buf[:self.total] != etx)
        assert len(bad) == 0, "%s: first wrong wire byte at %d of %d" % (tag, int(bad[0]), self.total)
        assert (buf[self.total:] == S.FILL).all(), tag
        return buf[:self.total]


@pytest.mark.parametrize("role", [False, True])
def test_ext_send_sets_rsv1_on_first_frames_only(dev, role):
    src = SC.source()
    conns = [[(0, 0, 0x41), (10, 5, 0x42), (100, 300, 0x41), (50, 1000, 1), (7, 0, O.SKIP), (2000, 700, 0x1F2), (9, 9, 0x4A)],
             [(300, 40000, 0x42), (5, 70, 2)], [], [(0, 20, 0x41), (len(src), 1, 0x41)], [(64, 4000, 0x41)]]
    frags = [130 + 4 * role, 4100, 100, 100, 7 + 4 * role]
    mm = 7
    keys = SC.keys_for(dict(role=role, conns=conns), mm)
    c = SendCall(dev, src, conns, frags, keys, mm, flags=1)
    c.run()
    tx = c.check("ext send, flag 1")
    assert int(c.exp[3]["n_frames"][0]) >= 3 + 6 and int(c.exp[3]["n_frames"][4]) == 800 and int(c.exp[3]["status"][3]) == S.ERR_RANGE
    plain = np.asarray(S.batch(src, conns, frags, keys, mm)[0], np.uint8)
    marked = [int(c.exp[2][s * mm + i]) for s, cn in enumerate(conns) if s != 3 for i, e in enumerate(cn) if e[2] != O.SKIP and e[2] & 0x40]
    assert [int(d) for d in np.flatnonzero(tx != plain)] == sorted(marked) and len(marked) == 7
    # flag 0: websocketframeBatchSendDevice's bytes, through both entry points
    z = SendCall(dev, src, conns, frags, keys, mm, flags=0)
    z.run()
    a = z.check("ext send, flag 0").copy()
    z.tx.fill_(S.FILL)
    z.run(ext=False)
    assert np.array_equal(z.check("plain send"), a) and np.array_equal(a, plain)


def chain_inputs():
    rng = np.random.default_rng(14)
    bodies = [IC.text(rng, int(n)) for n in (900, 3000, 130, 5000, 64, 2000)] + [DC.rnd(15, 800), b"", IC.text(rng, 20), b"k" * 1500]
    src, spans = place(bodies)
    conns = [[spans[0] + (1,), spans[6] + (2,), spans[1] + (1,)], [spans[3] + (2,), spans[7] + (1,), spans[8] + (1,), spans[9] + (2,)],
             [spans[2] + (1,), (0, 0, O.SKIP), spans[4] + (2,), spans[5] + (1,)]]
    return bodies, src, conns


class Chain:
    """deflate -> map -> ext send on one set of buffers"""

    def __init__(self, dev, src, conns, frags):
        self.d = Call(dev, src, conns, min_len=0, max_msgs=4)
        self.nseg, self.mm = self.d.nseg, 4
        self.lst = T(np.full(24 * self.nseg * self.mm, S.FILL, np.uint8), dev)
        self.frags = T(np.asarray(frags, np.uint32), dev).view(torch.int32)
        self.cap = sum(int(c) for c in self.d.caps) + 14 * self.nseg * self.mm * 8
        self.tx = torch.full((self.cap,), S.FILL, dtype=torch.uint8, device=dev)
        self.tx_off = T(np.full(self.nseg + 1, NONE64, np.uint64), dev).view(torch.int64)
        self.res = T(np.full(self.nseg * 32, S.FILL, np.uint8), dev)

    def run(self, stream=None):
        d = self.d
        d.run(stream)
        W.batch_send_list_from_deflated_device(d.msg, d.nmsg, self.mm, d.mres[:24 * self.nseg * self.mm], self.lst, stream=stream)
        W.batch_send_ext_device(d.dst, self.lst, d.nmsg, self.mm, self.tx, self.tx_off, self.res, frag_size=self.frags, flags=1,
                                stream=stream)

    def outputs(self):
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (self.d.dst, self.d.mres, self.lst, self.tx, self.tx_off.view(torch.uint8), self.res)]

    def refill(self):
        for t in (self.d.dst, self.d.mres, self.lst, self.tx, self.res):
            t.fill_(O.FILL if t is self.d.dst or t is self.d.mres else S.FILL)
        self.tx_off.view(torch.uint8).fill_(0xEE)


def test_full_chain_back_to_the_originals(dev):
    """originals -> deflate -> map -> ext send (server role, the echo test's fragment sizes) ->
    reassemble -> inflate list -> inflate: DEFLATED and PLAIN messages alike come back"""
    bodies, src, conns = chain_inputs()
    ch = Chain(dev, src, conns, [1464, S.FRAG_DEFAULT, 1464])
    ch.run()
    ch.d.check("chain deflate")
    dst, mres, lst, tx, tx_off, res = ch.outputs()
    rec = ch.d.records()
    # the wire is the model's over the rooms
    send_conns = [[O.send_entry(int(ch.d.msg_np[s * 4 + i]["type"]), int(rec[s * 4 + i]["status"]), int(rec[s * 4 + i]["out_off"]),
                                int(rec[s * 4 + i]["out_len"])) for i in range(len(c))] for s, c in enumerate(conns)]
    etx, eoff, _, eres = O.send_ext(dst, send_conns, [1464, S.FRAG_DEFAULT, 1464], None, 4)
    total = int(eoff[-1])
    assert np.array_equal(tx_off.view(np.uint64), eoff) and np.array_equal(tx[:total], etx) and (tx[total:] == S.FILL).all()
    assert np.array_equal(res.view(S.RES_DTYPE), eres) and int(eres["n_frames"].max()) >= 3
    # the receive side
    nseg, mf = 3, 16
    wire = torch.zeros(total + W.BATCH_PAD, dtype=torch.uint8, device=dev)
    wire[:total] = ch.tx[:total]
    t64 = lambda a: T(np.array(a, np.uint64), dev).view(torch.int64)  # noqa: E731
    so, sl = [int(v) for v in eoff[:-1]], [int(eoff[s + 1] - eoff[s]) for s in range(nseg)]
    out = torch.full((total + 256,), 0x55, dtype=torch.uint8, device=dev)
    desc = torch.zeros(nseg * 32 * mf, dtype=torch.uint8, device=dev)
    rres = torch.zeros(nseg * 16, dtype=torch.uint8, device=dev)
    msg = torch.zeros(nseg * 32 * mf, dtype=torch.uint8, device=dev)
    nmsg = torch.zeros(nseg, dtype=torch.int32, device=dev)
    W.batch_reassemble_device(wire, t64(so), t64(sl), mf, desc, rres, out, msg, nmsg, out_off=t64(so))
    ilst = torch.zeros(nseg * 24 * mf, dtype=torch.uint8, device=dev)
    W.batch_inflate_list_from_messages_device(wire, desc, msg, nmsg, mf, ilst)
    room = 12000
    back = torch.full((nseg * room,), 0x33, dtype=torch.uint8, device=dev)
    imres = torch.zeros(nseg * mf * 24, dtype=torch.uint8, device=dev)
    ires = torch.zeros(nseg * 24, dtype=torch.uint8, device=dev)
    W.batch_inflate_device(out, ilst, nmsg, mf, back, t64([s * room for s in range(nseg)]), t64([room] * nseg), imres, ires)
    torch.cuda.synchronize()
    nm = nmsg.cpu().numpy()
    md = msg.cpu().numpy().view(W.MSG_DTYPE)
    il = ilst.cpu().numpy().view(W.INFLATE_MSG_DTYPE)
    im = imres.cpu().numpy().view(W.INFLATE_MSGRES_DTYPE)
    assert (ires.cpu().numpy().view(W.INFLATE_RES_DTYPE)["status"] == W.INFLATE_OK).all()
    body, flat = out.cpu().numpy(), back.cpu().numpy()
    kinds = set()
    for s, c in enumerate(conns):
        sent = [(i, e) for i, e in enumerate(c) if e[2] != O.SKIP]
        assert int(nm[s]) == len(sent)
        for j, (i, (o, n, t)) in enumerate(sent):
            orig = bytes(src[o:o + n])
            st = int(rec[s * 4 + i]["status"])
            kinds.add(st)
            if st == O.DEFLATED:
                assert int(il[s * mf + j]["kind"]) == W.INFLATE_RAW and int(im[s * mf + j]["out_len"]) == n
                assert bytes(flat[int(im[s * mf + j]["out_off"]):][:n]) == orig
            else:
                assert st == O.PLAIN and int(il[s * mf + j]["kind"]) == W.INFLATE_SKIP
                assert int(md[s * mf + j]["len"]) == n and bytes(body[int(md[s * mf + j]["out_off"]):][:n]) == orig
    assert kinds == {O.DEFLATED, O.PLAIN}


def test_chain_captured_and_replayed(dev):
    bodies, src, conns = chain_inputs()
    ch = Chain(dev, src, conns, [1464, S.FRAG_DEFAULT, 200])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ch.run(st)                                          # the warm call, and the eager result
        eager = ch.outputs()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            ch.run(st)
    ch.refill()
    torch.cuda.synchronize()
    g.replay()
    for a, b in zip(eager, ch.outputs()):
        assert np.array_equal(a, b)
    ch.d.check("replay")


def test_two_streams_equal_serial_runs(dev, table):
    small = [b for _, b in table if len(b) <= 4096]
    src, spans = place(small)
    rng = np.random.default_rng(3)
    a = Call(dev, src, ragged(spans, rng))
    b = Call(dev, src, ragged(spans[::-1], rng), min_len=100)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a.run(s1)
    with torch.cuda.stream(s2):
        b.run(s2)
    a.check("stream 1")
    b.check("stream 2")


@pytest.fixture(scope="module")
def arenas(dev):
    H.need_memory(torch, pytest)
    a, b = H.Arena(dev), H.Arena(dev)
    yield a, b
    del a.t, b.t
    torch.cuda.empty_cache()


def test_offsets_past_4gib(dev, arenas):
    """bodies that straddle 2^32 in a sparse source arena, rooms that straddle 2^32 in a sparse
    destination arena: results and rooms are the host twin's on the small images, moved; an offset
    cut to 31 or 32 bits reads or writes the windows' low aliases (sentinels), and is seen"""
    sa, ta = arenas
    rng = np.random.default_rng(4)
    small = np.frombuffer(IC.text(rng, 3000) + DC.rnd(5, 500) + IC.text(rng, 1500), np.uint8).copy()
    at = 2000                                            # this source byte lies at 2^32
    high = H.place(H.B32, at)
    conns = [[(0, 3000, 1), (1990, 20, 2)], [(3000, 500, 2), (3500, 1500, 1)]]
    mm, nseg = 2, 2
    msg, nmsg, _ = S.pack(conns, mm)
    caps = np.array([3000, 20, 500, 1500], np.uint64)
    offs = np.array([64, 64 + 3000 + 33, 64 + 3000 + 33 + 20 + 7, 64 + 3000 + 33 + 20 + 7 + 500 + 5], np.uint64)
    dlen = int(offs[-1] + caps[-1]) + 64
    edst, emres = host_twin(small, msg.view(O.MSG_DTYPE), nmsg.view(np.uint32), mm, 0, dlen, offs, caps)
    dhigh = H.place(H.B32, 1500)                         # room 0 straddles 2^32
    placed_src = sa.put(high, small)
    placed_dst = ta.put(dhigh, np.full(dlen, O.FILL, np.uint8))
    hm = msg.view(O.MSG_DTYPE).copy()
    hm["src_off"] += np.uint64(high)
    mres = torch.full((24 * nseg * mm + 24,), O.FILL, dtype=torch.uint8, device=dev)
    W.batch_deflate_device(sa.view(high, len(small)), T(hm, dev), T(nmsg, dev).view(torch.int32), mm, ta.view(dhigh, dlen),
                           T(offs + np.uint64(dhigh), dev).view(torch.int64), T(caps, dev).view(torch.int64),
                           mres[:24 * nseg * mm], src_len=high + len(small))
    torch.cuda.synchronize()
    got = mres.cpu().numpy()
    want = emres.copy()
    w = want[:24 * nseg * mm].view(O.MSGRES_DTYPE)
    w["out_off"] += np.uint64(dhigh)
    assert np.array_equal(got, want)
    assert {int(v) for v in w["status"]} == {O.DEFLATED, O.PLAIN}
    ta.check(placed_dst, edst, "rooms past 2^32")
    sa.check(placed_src, small, "source past 2^32")


def test_argument_errors_launch_nothing(dev):
    src, spans = place([IC.text(np.random.default_rng(1), 400)])
    c = Call(dev, src, [[spans[0] + (1,)]])
    lib = _lib.load_pmd_lib()
    p = dict(src=c.src.data_ptr(), n=c.src.numel(), msg=c.msg.data_ptr(), nmsg=c.nmsg.data_ptr(), nseg=1, mm=1, min_len=0, flags=0,
             dst=c.dst.data_ptr(), off=c.off_t.data_ptr(), cap=c.cap_t.data_ptr(), mres=c.mres.data_ptr())

    def call(**kw):
        a = dict(p, **kw)
        return lib.websocketframeBatchDeflateDevice(a["src"], a["n"], a["msg"], a["nmsg"], a["nseg"], a["mm"], a["min_len"], a["flags"],
                                                    a["dst"], a["off"], a["cap"], a["mres"], None)
    for kw, word in ([(dict([(k, None)]), b"NULL") for k in ("src", "msg", "nmsg", "dst", "off", "cap", "mres")] +
                     [(dict(mm=0), b"max_msgs"), (dict(flags=1), b"flag"), (dict(msg=p["msg"] + 4), b"aligned"),
                      (dict(mres=p["mres"] + 4), b"aligned"), (dict(off=p["off"] + 4), b"aligned"), (dict(nmsg=p["nmsg"] + 2), b"aligned"),
                      (dict(nseg=1 << 16, mm=(1 << 14) + 1), b"2^30")]):
        assert call(**kw) < 0 and word in lib.websocketframeGpuLastError(), kw
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    assert lib.websocketframeBatchSendListFromDeflatedDevice(None, d.data_ptr(), 1, 1, d.data_ptr(), d.data_ptr(), None) < 0
    assert lib.websocketframeBatchSendListFromDeflatedDevice(d.data_ptr(), d.data_ptr(), 1, 0, d.data_ptr(), d.data_ptr(), None) < 0
    assert lib.websocketframeBatchSendExtDevice(d.data_ptr(), 64, d.data_ptr(), d.data_ptr(), 1, 1, None, None, 2, d.data_ptr(), 64,
                                                d.data_ptr(), None, d.data_ptr(), None) < 0
    assert b"websocketframeBatchSendExtDevice" in lib.websocketframeGpuLastError() and b"flag" in lib.websocketframeGpuLastError()
    torch.cuda.synchronize()
    assert bool((c.dst == O.FILL).all()) and bool((c.mres == O.FILL).all()) and not bool(d.any())
    c.run()
    assert [int(v) for v in c.check("after the refusals")] == [O.DEFLATED]
