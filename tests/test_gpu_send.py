"""websocketframeBatchSendDevice and websocketframeBatchSendListFromMessagesDevice on the device, bit
for bit against the sequential model (send_oracle.py): d_tx, d_tx_off, d_msg_tx_off, the results,
and a sentinel fill past min(total, capacity) (and in every slot the call does not own) untouched."""
import numpy as np
import pytest

import high_arena as H
import reasm_cases
import send_cases as SC
import send_oracle as S
from oracle_lib import oracle_reassemble
from util_amd import wsframe as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
NONE64 = 0xEEEEEEEEEEEEEEEE
TAIL = 4096                       # sentinel bytes kept behind every tx buffer


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def src():
    return SC.source()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)


class Call:
    """the device buffers of one batch; run() calls the library, check() holds every output
    against the model's"""

    def __init__(self, dev, src, conns, frags=None, keys=None, max_msgs=None, cap=None, tx_shift=0, exp=None, src_t=None):
        self.dev, self.nseg = dev, len(conns)
        msg, nmsg, self.mm = S.pack(conns, max_msgs)
        self.exp = exp or S.batch(src, conns, frags, keys, self.mm)
        self.total = int(self.exp[1][-1])
        self.cap = self.total if cap is None else cap
        self.src = T(src, dev) if src_t is None else src_t
        self.msg, self.nmsg = T(msg, dev), T(nmsg, dev)
        self.frags = None if frags is None else T(np.asarray(frags, np.uint32), dev)
        self.keys = None if keys is None else T(keys, dev)
        self.shift = tx_shift
        self.txbuf = torch.full((tx_shift + self.cap + TAIL,), S.FILL, dtype=torch.uint8, device=dev)
        self.tx_off = T(np.full(self.nseg + 2, NONE64, np.uint64), dev)
        self.moff = T(np.full(self.nseg * self.mm + 1, NONE64, np.uint64), dev)
        self.res = T(np.full(self.nseg * 32 + 32, S.FILL, np.uint8), dev)

    def run(self, stream=None):
        tx = self.txbuf[self.shift:self.shift + self.cap] if self.cap else None
        W.batch_send_device(self.src, self.msg, self.nmsg[:4 * self.nseg].view(torch.int32), self.mm, tx,
                            self.tx_off[:8 * (self.nseg + 1)], self.res[:32 * self.nseg], frag_size=self.frags, mask_key=self.keys,
                            msg_tx_off=self.moff[:8 * self.nseg * self.mm], tx_capacity=self.cap, stream=stream)

    def check(self, tag=""):
        torch.cuda.synchronize()
        etx, eoff, emoff, eres = self.exp
        got_off = self.tx_off.cpu().numpy().view(np.uint64)
        assert np.array_equal(got_off[:self.nseg + 1], eoff) and got_off[self.nseg + 1] == NONE64, tag
        res = self.res.cpu().numpy()
        print(tag, "total", self.total, "cap", self.cap, "frames", int(eres["n_frames"].sum()))
        assert np.array_equal(res[:32 * self.nseg].view(S.RES_DTYPE), eres), tag
        assert (res[32 * self.nseg:] == S.FILL).all(), tag
        moff = self.moff.cpu().numpy().view(np.uint64)
        assert np.array_equal(moff[:-1], emoff) and moff[-1] == NONE64, tag
        buf = self.txbuf.cpu().numpy()
        fit = min(self.total, self.cap)
        assert (buf[:self.shift] == S.FILL).all(), tag + ": bytes before d_tx written"
        bad = np.flatnonzero(buf[self.shift:self.shift + fit] != etx[:fit])
        assert len(bad) == 0, "%s: first wrong wire byte at %d of %d" % (tag, int(bad[0]), fit)
        assert (buf[self.shift + fit:] == S.FILL).all(), tag + ": bytes past min(total, capacity) written"


def run_case(dev, src, case, **kw):
    msg, nmsg, mm, keys, exp = SC.expect(case, src, kw.pop("max_msgs", None))
    c = Call(dev, src, case["conns"], case["frags"], keys, mm, exp=exp, **kw)
    c.run()
    c.check(case["name"])
    return c


@pytest.mark.parametrize("k", range(len(SC.directed_table())))
def test_directed_table(dev, src, k):
    run_case(dev, src, SC.directed_table()[k], tx_shift=k % 16)


@pytest.mark.parametrize("k", range(0, 24, 3))
def test_random_lists(dev, src, k):
    run_case(dev, src, SC.random_cases()[k], tx_shift=(5 * k) % 16)


@pytest.mark.parametrize("role", [False, True])
def test_4096_one_byte_messages_in_one_connection(dev, src, role):
    """more than 64 records per piece, more than 2048 between two piece pointers, 16 tiles of slots"""
    conns = [[(i * 7 % 1000, 1, 2) for i in range(4096)]]
    run_case(dev, src, dict(name="4096 x 1 B", conns=conns, frags=[S.FRAG_DEFAULT], role=role))


@pytest.mark.parametrize("role", [False, True])
def test_three_byte_stride_across_piece_edges(dev, src, role):
    """shard 1 over a 40 KiB message: every chunk holds several frames"""
    F = 7 if role else 3
    run_case(dev, src, dict(name="F = %d over 40 KiB" % F, conns=[[(3, 40960, 2)]], frags=[F], role=role), tx_shift=3)


@pytest.mark.parametrize("F", [S.FRAG_DEFAULT, 4100])
@pytest.mark.parametrize("role", [False, True])
def test_one_mib_message(dev, role, F):
    big = np.random.default_rng(8).integers(0, 256, (1 << 20) + 64, dtype=np.uint8)
    run_case(dev, big, dict(name="1 MiB, F = %d" % F, conns=[[(13, 1 << 20, 1)]], frags=[F], role=role))


def test_1000_connections_of_mixed_lists(dev, src):
    rng = np.random.default_rng(77)
    conns, frags = [], []
    for s in range(1000):
        c = []
        for _ in range(int(rng.integers(0, 6))):
            L = int(rng.choice([0, 1, 16, 125, 126, int(rng.integers(0, 600))]))
            kind = int(rng.integers(0, 30))
            so = int(rng.integers(0, SC.SRC_LEN - L))
            c.append((so, L, S.SKIP) if kind == 0 else ((SC.SRC_LEN, L + 1, 2) if kind == 1 else (so, L, 1 + kind % 2)))
        conns.append(c)
        frags.append(int(rng.choice([S.FRAG_DEFAULT, 2, 3, 50, 130, 1464])))
    for role in (False, True):
        c = run_case(dev, src, dict(name="1000 connections", conns=conns, frags=frags, role=role), max_msgs=7)
        st = set(int(v) for v in c.exp[3]["status"])
        assert st == {0, 1, 2}


PERIOD_1 = [[(11, 5, 2)], [], [(700, 0, 1)], [(3, 9, S.SKIP)], [(SC.SRC_LEN, 1, 2)], [(4321, 20, 1)], [(99, 13, 2)]]
PERIOD_3 = [[(11, 5, 2), (40, 20, 1), (7, 0, 2)], [], [(700, 17, 1)], [(3, 9, S.SKIP), (5, 1, 2)], [(8, 3, 1), (SC.SRC_LEN - 1, 2, 2), (9, 4, 2)],
            [(4321, 20, 1), (1, 1, S.SKIP), (77, 11, 1)], [(99, 13, 2), (100, 2, 2)]]


@pytest.mark.parametrize("role", [False, True])
@pytest.mark.parametrize("nseg,max_msgs,period", [(262145, 1, PERIOD_1), (87382, 3, PERIOD_3)])
def test_more_than_1024_blocks_and_tiles(dev, src, role, nseg, max_msgs, period):
    """262 145 connections of one slot: 1025 blocks of 256 connections, so every thread of the
    one-block scan of the block sums (u64) takes two; 87 382 connections of three slots: 1025 tiles
    with connections across the tile edges, so every thread of the one-block scan of the tile
    summaries takes two. Messages of 0 to 20 bytes, SKIP entries, a range error, and a fragment
    size that carries no byte on the last connection of the period of seven, which is repeated. The
    model runs on one period; its per-connection answers are repeated and the offsets are the
    running sum of the repeated lengths, which is exact: a connection stands alone."""
    P = len(period)
    reps, rest = nseg // P, nseg % P
    tile = lambda a, per=1: np.tile(a, reps + 1)[:nseg * per]
    pfrags = [S.FRAG_DEFAULT, 130, S.FRAG_DEFAULT, 50, S.FRAG_DEFAULT, 16, 2]
    pkeys = SC.keys_for(dict(role=role, conns=period), max_msgs)
    ptx, poff, pmoff, pres = S.batch(src, period, pfrags, pkeys, max_msgs)
    assert [int(v) for v in pres["status"]] == [0, 0, 0, 0, S.ERR_RANGE, 0, S.ERR_FRAGMENT_SIZE] and int(poff[-1]) > 0
    off = np.concatenate([[0], np.cumsum(tile(np.diff(poff.astype(np.int64))))]).astype(np.uint64)
    moff = tile(pmoff - np.repeat(poff[:-1], max_msgs), max_msgs) + np.repeat(off[:-1], max_msgs)
    moff[tile(pmoff, max_msgs) == NONE64] = NONE64            # the slots past a connection's count
    exp = (np.concatenate([np.tile(ptx, reps), ptx[:int(poff[rest])]]), off, moff, tile(pres))
    assert len(exp[0]) == int(off[-1]) < 8 << 20
    c = Call(dev, src, (period * (reps + 1))[:nseg], tile(pfrags), None if pkeys is None else tile(pkeys, max_msgs), max_msgs, exp=exp)
    c.run()
    c.check("%d connections of %d, role %d" % (nseg, max_msgs, role))


@pytest.mark.parametrize("role", [False, True])
def test_source_phases_and_fan_out(dev, src, role):
    """src_off at all 16 phases (and d_tx at several), then one body fanned out to 64 connections"""
    conns = [[(1000 + p, 700 + p, 2)] for p in range(16)]
    for shift in (0, 1, 9, 15):
        run_case(dev, src, dict(name="phase", conns=conns, frags=[S.FRAG_DEFAULT] * 16, role=role), tx_shift=shift)
    fan = [[(4321, 5000, 1)] for _ in range(64)]
    run_case(dev, src, dict(name="fan-out", conns=fan, frags=[S.FRAG_DEFAULT] * 32 + [1464] * 32, role=role))


@pytest.mark.parametrize("role", [False, True])
def test_capacity_cuts(dev, src, role):
    """tx_capacity 0 (d_tx NULL), mid-header, mid-body, exactly at a piece edge, total - 1"""
    case = dict(name="cuts", conns=[[(0, 70000, 2), (5, 300, 1)], [(9, 20000, 2)], [(1, 0, 1), (2, 126, 2)]],
                frags=[S.FRAG_DEFAULT, 4100, 100], role=role)
    msg, nmsg, mm, keys, exp = SC.expect(case, src)
    total = int(exp[1][-1])
    for cap in (0, 1, 5, 9, 4000, 16384, 32768, 16384 - 7, int(exp[1][1]) + 1, total - 1, total, total + 100):
        for shift in (0, 7):
            c = Call(dev, src, case["conns"], case["frags"], keys, mm, cap=cap, tx_shift=shift, exp=exp)
            c.run()
            c.check("cap %d shift %d" % (cap, shift))


def test_arguments(dev, src):
    from util_amd import _lib
    lib = _lib.load_send_lib()
    c = Call(dev, src, [[(0, 10, 2)]])
    good = dict(src=c.src.data_ptr(), n=c.src.numel(), msg=c.msg.data_ptr(), nmsg=c.nmsg.data_ptr(), nseg=1, mm=1, flags=0,
                tx=c.txbuf.data_ptr(), cap=c.cap, off=c.tx_off.data_ptr(), res=c.res.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.websocketframeBatchSendDevice(a["src"], a["n"], a["msg"], a["nmsg"], a["nseg"], a["mm"], None, None, a["flags"],
                                                 a["tx"], a["cap"], a["off"], None, a["res"], torch.cuda.current_stream().cuda_stream)
    for kw, word in ((dict(flags=1), b"flag"), (dict(mm=0), b"max_msgs"), (dict(src=None), b"NULL"), (dict(msg=None), b"NULL"),
                     (dict(nmsg=None), b"NULL"), (dict(tx=None), b"NULL"), (dict(off=None), b"NULL"), (dict(res=None), b"NULL"),
                     (dict(n=(1 << 56) + 1), b"src_len"), (dict(nseg=1 << 16, mm=1 << 15), b"2^30")):
        assert call(**kw) < 0 and word in lib.websocketframeGpuLastError(), kw
    torch.cuda.synchronize()
    assert bool((c.txbuf == S.FILL).all()) and bool((c.res == S.FILL).all())
    assert call(nseg=0) == 0                            # writes d_tx_off[0] = 0 only
    torch.cuda.synchronize()
    off = c.tx_off.cpu().numpy().view(np.uint64)
    assert off[0] == 0 and off[1] == NONE64 and bool((c.txbuf == S.FILL).all()) and bool((c.res == S.FILL).all())


@pytest.mark.parametrize("role", [False, True])
def test_captured_graph_replay(dev, src, role):
    """captured after one warm call; the bodies, the lists, the counts and (client role, d_tx at an
    odd phase) the keys change between replays"""
    rng = np.random.default_rng(4)
    variants = []
    for v in range(3):
        conns = [[(int(rng.integers(0, 1000)), int(rng.choice([0, 5, 126, 3000, 40000])), 1 + i % 2) for i in range(int(rng.integers(0, 5)))]
                 for _ in range(6)]
        keys = rng.integers(0, 1 << 32, 24, dtype=np.uint64).astype(np.uint32) if role else None
        variants.append((rng.integers(0, 256, SC.SRC_LEN, dtype=np.uint8), conns, keys))
    frags = [S.FRAG_DEFAULT, 130, 4100, 3 + 4 * role, 1464, 65546]
    cap = 1500000                                   # (a 40000-byte message in 7-byte frames is 280000 wire bytes)
    c = Call(dev, variants[0][0], variants[0][1], frags, variants[0][2], 4, cap=cap, tx_shift=5 if role else 0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        c.run(stream)                                   # the warm call
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            c.run(stream)
    for body, conns, keys in variants[::-1]:
        msg, nmsg, _ = S.pack(conns, 4)
        c.src.copy_(T(body, dev))
        c.msg.copy_(T(msg, dev))
        c.nmsg.copy_(T(nmsg, dev))
        if role:
            c.keys.copy_(T(keys, dev))
        c.txbuf.fill_(S.FILL)
        c.moff.fill_(S.FILL)                            # (slots an earlier replay's lists owned)
        c.exp = S.batch(body, conns, frags, keys, 4)
        c.total = int(c.exp[1][-1])
        assert c.total <= cap
        torch.cuda.synchronize()
        g.replay()
        c.check("replay")


@pytest.mark.parametrize("names", [("mixed", "zero_len"), ("boundary", "mixed")])
def test_echo_over_a_reassembly_call(dev, names):
    """reassemble two fixture streams as two connections whose output regions lie elsewhere and in
    the other order (d_out_off), map the message descriptors to a send list on the device, send:
    the list is what the descriptors say — out_off counts from d_out, the region's offset included —
    and the wire bytes are the model's over reassembly's output"""
    wires = [reasm_cases.build(nm)[0] for nm in names]
    gap, mf = 37, 64
    wire = np.concatenate([wires[0], np.zeros(gap, np.uint8), wires[1]])
    n = len(wire)
    so, sl = [0, len(wires[0]) + gap], [len(wires[0]), len(wires[1])]
    oo = [len(wires[1]) + 101, 7]                      # connection 0's region behind connection 1's
    od, orr, oms, oreg, _, _ = oracle_reassemble(wire, so, sl, mf, out_off=oo)
    d = torch.zeros(n + W.BATCH_PAD, dtype=torch.uint8, device=dev)
    d[:n] = T(wire, dev)
    out = torch.full((n + 256,), 0x55, dtype=torch.uint8, device=dev)
    desc = torch.zeros(2 * 32 * mf, dtype=torch.uint8, device=dev)
    res = torch.zeros(32, dtype=torch.uint8, device=dev)
    msg = torch.zeros(2 * 32 * mf, dtype=torch.uint8, device=dev)
    nmsg = torch.zeros(2, dtype=torch.int32, device=dev)
    t64 = lambda a: T(np.array(a, np.uint64), dev).view(torch.int64)  # noqa: E731
    W.batch_reassemble_device(d, t64(so), t64(sl), mf, desc, res, out, msg, nmsg, out_off=t64(oo))
    lst = T(np.full(2 * mf * 24 + 24, S.FILL, np.uint8), dev)
    W.batch_send_list_from_messages_device(desc, msg, nmsg, mf, lst[:2 * 24 * mf])
    torch.cuda.synchronize()
    body = out.cpu().numpy()
    got = lst.cpu().numpy()
    assert (got[2 * 24 * mf:] == S.FILL).all()
    conns = []
    for s in range(2):
        want = []
        for (o, ln, first, _nf, complete, cont) in oms[s]:
            t = int(od[s * mf + first]["type"])
            want.append((o, ln, t) if complete and not cont and t in (1, 2) else (0, 0, S.SKIP))
        mine = got[s * 24 * mf:(s + 1) * 24 * mf]
        assert (mine[24 * len(want):] == S.FILL).all(), "slots past the count written"
        rec = mine[:24 * len(want)].view(S.MSG_DTYPE)
        assert [(int(r["src_off"]), int(r["len"]), int(r["type"])) for r in rec] == want and not rec["reserved"].any()
        assert any(t != S.SKIP and o >= oo[s] for o, _, t in want)
        for o, ln, t in want:
            if t != S.SKIP:                             # the entry points at the message's body
                assert np.array_equal(body[o:o + ln], oreg[s][1][o - oo[s]:o - oo[s] + ln])
        conns.append(want)
    # the echo: d_out as d_src, d_nmsg and max_frames reused
    c = Call(dev, body, conns, [1464, S.FRAG_DEFAULT], None, mf, src_t=out)
    c.msg, c.nmsg = lst, nmsg.view(torch.uint8)
    c.run()
    c.check("echo " + "+".join(names))


# ---------------------------------------------------------------------------------- past 2^32

@pytest.fixture(scope="module")
def arenas(dev):
    H.need_memory(torch, pytest)
    a, b = H.Arena(dev), H.Arena(dev)
    yield a, b
    del a.t, b.t
    torch.cuda.empty_cache()


def test_offsets_past_4gib(dev, arenas):
    """Connection 0 sends one message of 2^32 + 20000 bytes from the bottom of a sparse source arena
    in 4096-byte fragments: its wire positions, frame indices times the stride and piece indices pass
    2^32. The connections after it read bodies that straddle 2^32 in the source arena (src_off past
    2^32) and their bytes lie past 2^32 in d_tx. Their bytes, offsets and results are the model's
    on the small source, moved by connection 0's closed-form length; connection 0's bytes are held
    against the source on the device, frame by frame. An offset cut to 31 or 32 bits reads the source
    window's low aliases (sentinels) or writes into connection 0's bytes: both are seen."""
    sa, ta = arenas
    F, shard, stride = 4100, 4096, 4100
    L0 = H.B32 + 20000                                  # (inside src_len; its end overlaps the window: fan-out)
    frames0, wire0 = S.closed_form(L0, F, False)
    last = L0 - (frames0 - 1) * shard
    small = SC.source()[:70000]
    at = 30001                                          # this byte of the small source lies at 2^32
    high = H.place(H.B32, at)
    step = 1 << 26
    for a in range(0, L0 + (1 << 20), step):            # the source below the window: address-dependent bytes
        sa.t[a:a + step] = sa.sentinel(a, a + step)
    placed = sa.put(high, small)
    conns = [[(0, 70000, 2)], [(at - 8, 16, 1), (at, 0, 2), (at + 1, 4000, 2)], [(5, 0, S.SKIP), (at - 300, 600, 1)]]
    frags = [S.FRAG_DEFAULT, 100, 1464]
    etx, eoff, emoff, eres = S.batch(small, conns, frags, None, 3)
    all_conns = [[(0, L0, 2)]] + [[(high + o, ln, t) for o, ln, t in c] for c in conns]
    msg, nmsg, mm = S.pack(all_conns, 3)
    total = wire0 + len(etx)
    ta.t[:total + 4096].fill_(S.FILL)
    tx_off = T(np.full(6, NONE64, np.uint64), dev)
    moff = T(np.full(4 * 3 + 1, NONE64, np.uint64), dev)
    res = T(np.full(4 * 32 + 32, S.FILL, np.uint8), dev)
    W.batch_send_device(sa.t, T(msg, dev), T(nmsg, dev).view(torch.int32), 3, ta.t[:total], tx_off[:40], res[:128],
                        frag_size=T(np.array([F] + frags, np.uint32), dev).view(torch.int32), msg_tx_off=moff[:96],
                        tx_capacity=total, src_len=high + len(small))
    torch.cuda.synchronize()
    got_off = tx_off.cpu().numpy().view(np.uint64)
    assert [int(v) for v in got_off[:5]] == [0] + [wire0 + int(v) for v in eoff] and got_off[5] == NONE64
    r = res.cpu().numpy()
    assert (r[128:] == S.FILL).all()
    r = r[:128].view(S.RES_DTYPE)
    assert tuple(int(v) for v in r[0]) == (wire0, frames0, 1, 0, S.NONE, 0) and np.array_equal(r[1:], eres)
    m = moff.cpu().numpy().view(np.uint64)
    want_m = np.full(13, NONE64, np.uint64)
    want_m[0] = 0
    want_m[3:12] = np.where(emoff == NONE64, emoff, emoff + np.uint64(wire0))
    assert np.array_equal(m, want_m)
    # the connections past 2^32, the sentinel behind them, the source untouched with its aliases
    tail = ta.t[wire0:total + 4096].cpu().numpy()
    bad = np.flatnonzero(tail[:len(etx)] != etx)
    assert len(bad) == 0, "first wrong byte past 2^32 at %d of %d" % (int(bad[0]) if len(bad) else -1, len(etx))
    assert (tail[len(etx):] == S.FILL).all()
    sa.check(placed, small, "the source window")
    # connection 0: every full frame is {0x02 or 0x00, 126, 0x10, 0x00} + 4096 source bytes
    nfull = frames0 - 1
    per = 1 << 16                                       # frames per compared slab
    for f0 in range(0, nfull, per):
        k = min(per, nfull - f0)
        fr = ta.t[f0 * stride:(f0 + k) * stride].view(k, stride)
        assert torch.equal(fr[:, 4:], sa.t[f0 * shard:(f0 + k) * shard].view(k, shard)), "frames from %d" % f0
        hd = fr[:, :4].cpu().numpy()
        assert (hd[:, 1:] == [126, 0x10, 0x00]).all() and (hd[1 if f0 == 0 else 0:, 0] == 0).all(), "headers from %d" % f0
    assert int(ta.t[0]) == 2
    lastf = ta.t[nfull * stride:wire0].cpu().numpy()
    assert len(lastf) == 4 + last and list(lastf[:4]) == [0x80, 126, last >> 8, last & 255]
    assert torch.equal(ta.t[nfull * stride + 4:wire0], sa.t[nfull * shard:L0])
